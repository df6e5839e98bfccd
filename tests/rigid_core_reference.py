"""The rigid core (DESIGN.md "Rigid core") restated in numpy fp64, operation for operation, so that its results can be compared
bit for bit: the 16 moments and the squared residual over the contract's partition (runs of 256 pairs, the wave butterfly,
tree4, then the chain's left-to-right fold or the strided fold of k_icp_fold / k_rigid_fold), the Jacobi SVD and the Kabsch
solve of o3dr_rigid_solve.h scalar by scalar, and the samplers' splitmix64 / draw3.  numpy never fuses a multiply-add, its
sqrt and division are correctly rounded, so every operation rounds as the library's does."""
import numpy as np

RIGID_N, RIGID_SA, RIGID_SB, RIGID_SAB, RIGID_FIELDS = 0, 1, 4, 7, 16
RUN, WAVE, FOLD_THREADS, CHAIN_THREADS = 256, 64, 1024, 1024
M64 = (1 << 64) - 1


# ---- the sampler ------------------------------------------------------------------------------------------------------------
def splitmix64(x):
    z = (int(x) + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw3(seed, key, h, m):
    """the three local indices (0 .. m - 1) of hypothesis h of the stream splitmix64(seed ^ key)"""
    S = splitmix64((int(seed) ^ int(key)) & M64)
    return [(((splitmix64((S + 3 * h + k) & M64) >> 32) * m) >> 32) for k in range(3)]


# ---- the sums ---------------------------------------------------------------------------------------------------------------
def pair_finite(src, tgt):
    return np.isfinite(np.asarray(src, np.float32).reshape(-1, 3)).all(1) & np.isfinite(np.asarray(tgt, np.float32).reshape(-1, 3)).all(1)


def moment_fields(src, tgt, used, c0):
    """[n, 16] fp64: rigid_moments of every pair (zeros where not used)"""
    s = np.asarray(src, np.float32).reshape(-1, 3).astype(np.float64)
    t = np.asarray(tgt, np.float32).reshape(-1, 3).astype(np.float64)
    used = np.asarray(used, bool)
    c0 = np.asarray(c0, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.where(used[:, None], s - c0, 0.0)
        b = np.where(used[:, None], t - c0, 0.0)
        v = np.zeros((len(s), RIGID_FIELDS))
        v[:, RIGID_N] = used
        v[:, RIGID_SA:RIGID_SA + 3] = a
        v[:, RIGID_SB:RIGID_SB + 3] = b
        for j in range(3):
            for k in range(3):
                v[:, RIGID_SAB + 3 * j + k] = a[:, j] * b[:, k]
    return v


def residual_field(T, src, tgt, used):
    """[n, 1] fp64: rigid_residual2 at T (12 fp64, 3 x 4 row-major) of every used pair, zero elsewhere"""
    s = np.asarray(src, np.float32).reshape(-1, 3).astype(np.float64)
    t = np.asarray(tgt, np.float32).reshape(-1, 3).astype(np.float64)
    T = np.asarray(T, np.float64).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        e = [((T[4 * r] * s[:, 0] + T[4 * r + 1] * s[:, 1]) + T[4 * r + 2] * s[:, 2]) + T[4 * r + 3] - t[:, r] for r in range(3)]
        r2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
    return np.where(np.asarray(used, bool), r2, 0.0)[:, None]


def wave_sum(x):
    """the butterfly of wave_sum_f64 over axis 0 (64 lanes): x[:32] + x[32:], then halves down to one"""
    x = np.asarray(x, np.float64)
    assert x.shape[0] == WAVE
    for half in (32, 16, 8, 4, 2, 1):
        x = x[:half] + x[half:2 * half]
    return x[0]


def run_partials(v, threads=RUN):
    """[n, F] -> [n_runs, F]: every run of 256 rows (the last one zero-padded; `threads`: padded to whole workgroups of that
    many rows) through wave_fields and tree4"""
    v = np.asarray(v, np.float64)
    n, F = v.shape
    total = max(-(-n // threads) * threads, threads)
    p = np.zeros((total, F))
    p[:n] = v
    w = np.moveaxis(p.reshape(total // RUN, 4, WAVE, F), 2, 0)  # [lane, run, wave, F]
    with np.errstate(invalid="ignore", over="ignore"):
        ws = wave_sum(w)
        return (ws[:, 0] + ws[:, 1]) + (ws[:, 2] + ws[:, 3])


def fold_chain(partials):
    """k_pose_chain / k_graph_moments: the runs added left to right, from 0.0"""
    tot = np.zeros(partials.shape[1])
    with np.errstate(invalid="ignore", over="ignore"):
        for p in partials:
            tot = tot + p
    return tot


def fold_strided(partials):
    """fold_partials (k_icp_fold, k_rigid_fold): thread t of 1024 adds partials t, t + 1024, .. in order; a wave butterfly; the 16
    waves' slots added in order, from 0.0"""
    n, F = partials.shape
    s = np.zeros((FOLD_THREADS, F))
    with np.errstate(invalid="ignore", over="ignore"):
        for b0 in range(0, n, FOLD_THREADS):
            chunk = partials[b0:b0 + FOLD_THREADS]
            s[:len(chunk)] = s[:len(chunk)] + chunk
        t = np.zeros(F)
        for wv in range(FOLD_THREADS // WAVE):
            t = t + wave_sum(s[WAVE * wv:WAVE * (wv + 1)])
    return t


# ---- the solve (o3dr_rigid_solve.h, scalar by scalar) --------------------------------------------------------------------
def rigid_svd3(A_in):
    f = np.float64
    A = [[f(A_in[i][j]) for j in range(3)] for i in range(3)]
    V = [[f(1.0 if i == j else 0.0) for j in range(3)] for i in range(3)]
    for _sweep in range(64):
        rotated = False
        for p in range(2):
            for q in range(p + 1, 3):
                alpha, beta, gamma = f(0.0), f(0.0), f(0.0)
                for i in range(3):
                    alpha = alpha + A[i][p] * A[i][p]
                    beta = beta + A[i][q] * A[i][q]
                    gamma = gamma + A[i][p] * A[i][q]
                if not (abs(gamma) > f(1e-15) * np.sqrt(alpha * beta)):
                    continue
                rotated = True
                zeta = (beta - alpha) / (f(2.0) * gamma)
                t = (f(1.0) if zeta >= 0.0 else f(-1.0)) / (abs(zeta) + np.sqrt(f(1.0) + zeta * zeta))
                cs = f(1.0) / np.sqrt(f(1.0) + t * t)
                sn = cs * t
                for i in range(3):
                    ap, aq = A[i][p], A[i][q]
                    A[i][p] = cs * ap - sn * aq
                    A[i][q] = sn * ap + cs * aq
                    vp, vq = V[i][p], V[i][q]
                    V[i][p] = cs * vp - sn * vq
                    V[i][q] = sn * vp + cs * vq
        if not rotated:
            break
    order = [0, 1, 2]
    nrm = [np.sqrt(A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j]) for j in range(3)]
    for k in range(1, 3):  # insertion sort, descending
        m = k
        while m > 0 and nrm[order[m]] > nrm[order[m - 1]]:
            order[m], order[m - 1] = order[m - 1], order[m]
            m -= 1
    S = [nrm[order[k]] for k in range(3)]
    Vs = [[V[i][order[k]] for k in range(3)] for i in range(3)]
    U = [[(A[i][order[k]] / nrm[order[k]] if nrm[order[k]] > 0.0 else f(0.0)) for k in range(3)] for i in range(3)]
    return U, S, Vs


def rigid_solve(rec, c0):
    """-> (ok, T [12] fp64): T keeps zeros where the solve returns before writing it"""
    f = np.float64
    rec = [f(x) for x in rec]
    c0 = [f(x) for x in c0]
    T = np.zeros(12)
    with np.errstate(all="ignore"):
        n = rec[RIGID_N]
        ma = [rec[RIGID_SA + k] / n for k in range(3)]
        mb = [rec[RIGID_SB + k] / n for k in range(3)]
        H = [[rec[RIGID_SAB + 3 * j + k] - n * ma[j] * mb[k] for k in range(3)] for j in range(3)]
        U, S, V = rigid_svd3(H)
        if not (S[0] > 0.0) or not np.isfinite(S[0]) or not (S[1] > f(1e-12) * S[0]):
            return False, T
        U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1]
        U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1]
        U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1]
        detV = (V[0][0] * (V[1][1] * V[2][2] - V[1][2] * V[2][1]) - V[0][1] * (V[1][0] * V[2][2] - V[1][2] * V[2][0]) +
                V[0][2] * (V[1][0] * V[2][1] - V[1][1] * V[2][0]))
        d = [f(1.0), f(1.0), f(-1.0) if detV < 0.0 else f(1.0)]
        R = [[V[i][0] * d[0] * U[j][0] + V[i][1] * d[1] * U[j][1] + V[i][2] * d[2] * U[j][2] for j in range(3)] for i in range(3)]
        for i in range(3):
            t = c0[i] + mb[i]
            for j in range(3):
                t = t - R[i][j] * (c0[j] + ma[j])
            for j in range(3):
                T[4 * i + j] = R[i][j]
            T[4 * i + 3] = t
    return bool(np.isfinite(T[3]) and np.isfinite(T[7]) and np.isfinite(T[11])), T


# ---- whole fits -----------------------------------------------------------------------------------------------------------
def rigid_fit(src, tgt, used, fold, threads=RUN):
    """One fit as the library runs it: c0 = the first used tgt, the moments, the solve, the residuals at T over the same
    partition and fold.  fold: fold_strided (o3dr_estimate_rigid_transform) or fold_chain with threads=CHAIN_THREADS (the
    chain).  -> dict(n_used, rec [16], c0, ok, T [12], d2, rms); T is the zeros and rms 0 when there is no solve."""
    src = np.asarray(src, np.float32).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float32).reshape(-1, 3)
    used = np.asarray(used, bool) & pair_finite(src, tgt)
    n_used = int(used.sum())
    c0 = tgt[np.argmax(used)].astype(np.float64) if n_used else np.zeros(3)
    rec = fold(run_partials(moment_fields(src, tgt, used, c0), threads))
    out = dict(n_used=n_used, rec=rec, c0=c0, ok=False, T=np.zeros(12), d2=0.0, rms=0.0)
    assert rec[RIGID_N] == n_used
    if n_used < 3:
        return out
    out["ok"], out["T"] = rigid_solve(rec, c0)
    return out


def residual_rms(T, src, tgt, used, n_used, fold, threads=RUN):
    d2 = fold(run_partials(residual_field(T, src, tgt, used), threads))[0]
    return float(np.sqrt(d2 / np.float64(n_used))) if n_used > 0 else 0.0
