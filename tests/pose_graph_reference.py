"""The pose-graph refinement's contract (include/o3dr.h "pose graph") restated in numpy, on top of pose_chain_reference.

refine_ref: per-pair moments from the matching (chain_ref's `match`, or a brute force of its own), the edge formulas of
DESIGN.md "Pose-graph refinement", block-Jacobi preconditioned CG with the contract's iteration counts (the diagonal blocks
inverted by the library's own Cholesky, invert6, so that a block that is not positive definite is held and flagged as the
contract says) and the Cayley retraction.  The summation orders are numpy's, not the library's: poses agree to rounding, not bit for bit.  reverse=True
sums every pair's rows in the opposite order; the tests take the distance between the two runs as the floor of what rounding
alone moves.  direct_energy / direct_gradient evaluate the energy and its gradient per correspondence, without moments."""
import numpy as np

import pose_chain_reference as R

FIXED, FREE, FLOATING, REJECTED = range(4)  # O3DR_REFINE_*
FLAG_CG_STOPPED = 1
FLAG_SINGULAR = 2


# ---- small algebra --------------------------------------------------------------------------------------------------------
def hat(a):
    return np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])


def vee_skew(P):
    """(P12 - P21, P20 - P02, P01 - P10)"""
    return np.array([P[1, 2] - P[2, 1], P[2, 0] - P[0, 2], P[0, 1] - P[1, 0]])


def orthonormal(pose16):
    """rows 0..2 of the fp32 pose, Gram-Schmidt by rows -> (R fp64 3x3, t fp64 3)"""
    m = np.asarray(pose16, np.float32).reshape(4, 4).astype(np.float64)
    r1, r2 = m[0, :3], m[1, :3]
    e1 = r1 / np.sqrt((r1[0] * r1[0] + r1[1] * r1[1]) + r1[2] * r1[2])
    u = r2 - ((r2[0] * e1[0] + r2[1] * e1[1]) + r2[2] * e1[2]) * e1
    e2 = u / np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
    e3 = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])
    return np.stack([e1, e2, e3]), m[:3, 3].copy()


def cayley(w):
    """the rotation of the unit quaternion (1, w / 2) / |.|"""
    x, y, z = 0.5 * w[0], 0.5 * w[1], 0.5 * w[2]
    n = np.sqrt(1.0 + ((x * x + y * y) + z * z))
    q0, x, y, z = 1.0 / n, x / n, y / n, z / n
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - q0 * z), 2.0 * (x * z + q0 * y)],
                     [2.0 * (x * y + q0 * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - q0 * x)],
                     [2.0 * (x * z - q0 * y), 2.0 * (y * z + q0 * x), 1.0 - 2.0 * (x * x + y * y)]])


# ---- moments --------------------------------------------------------------------------------------------------------------
def pair_rows(off, xyz, status, i, j, idx, good, inlier=None):
    """-> (a, b) fp64 [n_used, 3] of pair (i, j) in row order, camera coordinates"""
    if status[i] > R.MATCHED or status[j] > R.MATCHED:
        return np.zeros((0, 3)), np.zeros((0, 3))
    rows = np.nonzero(good)[0]
    a = xyz[off[i]:off[i + 1]][rows]
    b = xyz[off[j]:off[j + 1]][idx[rows, 0].astype(np.int64)]
    use = np.isfinite(a).all(1) & np.isfinite(b).all(1)
    if inlier is not None:
        use &= np.asarray(inlier)[rows] != 0
    return a[use].astype(np.float64), b[use].astype(np.float64)


def moments(a, b):
    """dict(n, Sa, Sb, Saa, Sbb, Sab) of fp64 rows"""
    return dict(n=float(len(a)), Sa=a.sum(0), Sb=b.sum(0), Saa=a.T @ a, Sbb=b.T @ b, Sab=a.T @ b)


# ---- the edge formulas ----------------------------------------------------------------------------------------------------
def edge_energy(m, Ri, ti, Rj, tj):
    M = Ri.T @ Rj
    d = Ri.T @ (ti - tj)
    return (np.trace(m["Saa"]) + np.trace(m["Sbb"]) + m["n"] * (d @ d) + 2.0 * (d @ m["Sa"]) - 2.0 * (M * m["Sab"]).sum()
            - 2.0 * (d @ (M @ m["Sb"])))


def diag_block(n, S, SS):
    H = np.zeros((6, 6))
    H[:3, :3] = n * np.eye(3)
    H[:3, 3:] = -hat(S)
    H[3:, :3] = hat(S)
    H[3:, 3:] = np.trace(SS) * np.eye(3) - SS
    return H


def invert6(A):
    """graph_invert6 operation for operation: A = L L^T with the pivots in order (row i over j <= i, s -= L[i][k] L[j][k]
    with k ascending), L^-1 column by column by forward substitution, the inverse L^-T L^-1.  None: a pivot that is not
    > 0 or not finite - the block is not positive definite."""
    A = np.asarray(A, np.float64)
    L = np.zeros((6, 6))
    for i in range(6):
        for j in range(i + 1):
            s = A[i, j]
            for k in range(j):
                s = s - L[i, k] * L[j, k]
            if i == j:
                if not (s > 0.0) or not np.isfinite(s):
                    return None
                L[i, i] = np.sqrt(s)
            else:
                L[i, j] = s / L[j, j]
    Li = np.zeros((6, 6))
    for c in range(6):
        for i in range(c, 6):
            s = 1.0 if i == c else 0.0
            for k in range(c, i):
                s = s - L[i, k] * Li[k, c]
            Li[i, c] = s / L[i, i]
    inv = np.zeros((6, 6))
    for i in range(6):
        for j in range(6):
            s = 0.0
            for k in range(max(i, j), 6):
                s = s + Li[k, i] * Li[k, j]
            inv[i, j] = s
    return inv


def edge_terms(m, Ri, ti, Rj, tj):
    """-> (H_ij 6x6, g_i 6, g_j 6)"""
    M = Ri.T @ Rj
    d = Ri.T @ (ti - tj)
    e = Rj.T @ (ti - tj)
    n, Sa, Sb, Sab = m["n"], m["Sa"], m["Sb"], m["Sab"]
    I = np.eye(3)
    W = np.zeros((3, 3))
    for p in range(3):
        for q in range(3):
            W += Sab[p, q] * (hat(I[p]) @ M @ hat(I[q]))
    Hij = np.zeros((6, 6))
    Hij[:3, :3] = n * M
    Hij[:3, 3:] = -M @ hat(Sb)
    Hij[3:, :3] = hat(Sa) @ M
    Hij[3:, 3:] = -W
    Hij = -Hij
    P = Sab @ M.T
    Q = Sab.T @ M
    gi = np.concatenate([Sa + n * d - M @ Sb, np.cross(Sa, d) - vee_skew(P)])
    gj = -np.concatenate([M.T @ Sa + n * e - Sb, vee_skew(Q) + np.cross(Sb, e)])
    return Hij, gi, gj


# ---- the direct sums (no moments) -----------------------------------------------------------------------------------------
def direct_energy(rows, Rs, ts, prior_weight=0.0, prior_t=None, free=()):
    """rows: [(i, j, a, b)] -> sum |R_i a + t_i - R_j b - t_j|^2 (+ the prior term over `free`)"""
    E = 0.0
    for (i, j, a, b) in rows:
        r = a @ Rs[i].T + ts[i] - b @ Rs[j].T - ts[j]
        E += float((r * r).sum())
    for f in (free if prior_weight else ()):
        d = ts[f] - prior_t[f]
        E += prior_weight * float(d @ d)
    return E


def direct_gradient(rows, Rs, ts, free, prior_weight=0.0, prior_t=None):
    """the contract's g (half the derivative of the energy in the right perturbation) over the free frames, per correspondence"""
    g = {f: np.zeros(6) for f in free}
    for (i, j, a, b) in rows:
        r = a @ Rs[i].T + ts[i] - b @ Rs[j].T - ts[j]
        if i in g:
            ri = r @ Rs[i]
            g[i][:3] += ri.sum(0)
            g[i][3:] += np.cross(a, ri).sum(0)
        if j in g:
            rj = r @ Rs[j]
            g[j][:3] -= rj.sum(0)
            g[j][3:] -= np.cross(b, rj).sum(0)
    for f in (free if prior_weight else ()):
        g[f][:3] += prior_weight * (Rs[f].T @ (ts[f] - prior_t[f]))
    return g


# ---- the contract ---------------------------------------------------------------------------------------------------------
def refine_ref(desc, offsets, kp3, poses, status, pairs, fixed=None, prior_poses=None, prior_weight=0.0, gn_iterations=5,
               cg_iterations=32, min_pair_matches=3, ratio=0.5, max_distance=40, match=None, inlier=None, reverse=False):
    """-> dict(poses [F, 16] float32, T [F, 12] fp64, role, degree [F]; n_good, n_used, edge [P]; e_before, e_after [P];
    energy_before, energy_after, grad_before, grad_after, last_step, n_free, n_gauge, n_floating, n_rejected, n_edges,
    n_used_total, flags; rows [(i, j, a, b)] of the edges, for direct_energy).  match: {(i, j): (idx, good)} of an earlier
    run (chain_ref's), inlier: {(i, j): mask per query row} (robust_chain_ref's) or None: no filter."""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    off = np.asarray(offsets, np.int64)
    xyz = np.asarray(kp3, np.float32).reshape(-1, 3)
    poses = np.asarray(poses, np.float32).reshape(-1, 16)
    status = np.asarray(status, np.int32).reshape(-1)
    F = len(off) - 1
    pairs = [(int(i), int(j)) for (i, j) in np.asarray(pairs, np.int64).reshape(-1, 2)]
    P = len(pairs)
    fixed = np.zeros(F, bool) if fixed is None else np.asarray(fixed).astype(bool)
    w = float(prior_weight)
    prior_t = None if prior_poses is None else np.asarray(prior_poses, np.float32).reshape(-1, 16)[:, [3, 7, 11]].astype(np.float64)
    out = dict(n_good=np.zeros(P, np.int32), n_used=np.zeros(P, np.int32), edge=np.zeros(P, np.int32), e_before=np.zeros(P),
               e_after=np.zeros(P), rows=[], flags=0)
    # step 1 + 2: matching and moments
    mom = [None] * P
    for k, (i, j) in enumerate(pairs):
        if match is not None and (i, j) in match:
            idx, good = match[(i, j)]
        else:
            idx, dist = R.knn2_ref(desc[off[i]:off[i + 1]], desc[off[j]:off[j + 1]])
            good = R.good_ref(dist, ratio, max_distance)
        out["n_good"][k] = int(good.sum())
        a, b = pair_rows(off, xyz, status, i, j, idx, good, None if inlier is None else inlier[(i, j)])
        out["n_used"][k] = len(a)
        if status[i] <= R.MATCHED and status[j] <= R.MATCHED and len(a) >= min_pair_matches:
            out["edge"][k] = 1
            out["rows"].append((i, j, a, b))
            mom[k] = moments(a[::-1], b[::-1]) if reverse else moments(a, b)
    edges = [k for k in range(P) if out["edge"][k]]
    # step 3: roles
    degree = np.zeros(F, np.int32)
    adj = [[] for _ in range(F)]  # (edge, side) in pair-list order
    for k in edges:
        i, j = pairs[k]
        degree[i] += 1
        degree[j] += 1
        adj[i].append((k, 0))
        adj[j].append((k, 1))
    role = np.full(F, FIXED, np.int32)
    for f in range(F):
        if status[f] > R.MATCHED:
            role[f] = REJECTED
        elif status[f] == R.MATCHED and not fixed[f] and degree[f] > 0:
            role[f] = FREE
    if w == 0.0:
        comp = list(range(F))

        def find(x):
            while comp[x] != x:
                comp[x] = comp[comp[x]]
                x = comp[x]
            return x
        for k in edges:
            i, j = pairs[k]
            comp[find(i)] = find(j)
        has_gauge = {}
        for f in range(F):
            if role[f] == FIXED and degree[f] > 0:
                has_gauge[find(f)] = True
        for f in range(F):
            if role[f] == FREE and not has_gauge.get(find(f), False):
                role[f] = FLOATING
    free = [f for f in range(F) if role[f] == FREE]
    pos = {f: n for n, f in enumerate(free)}
    Rs, ts = [], []
    for f in range(F):
        Rf, tf = orthonormal(poses[f])
        Rs.append(Rf)
        ts.append(tf)

    def assemble():
        Hd = {f: np.zeros((6, 6)) for f in free}
        g = {f: np.zeros(6) for f in free}
        Hij, E = {}, np.zeros(P)
        for k in edges:
            i, j = pairs[k]
            m = mom[k]
            E[k] = edge_energy(m, Rs[i], ts[i], Rs[j], ts[j])
            H, gi, gj = edge_terms(m, Rs[i], ts[i], Rs[j], ts[j])
            Hij[k] = H
            if i in pos:
                Hd[i] += diag_block(m["n"], m["Sa"], m["Saa"])
                g[i] += gi
            if j in pos:
                Hd[j] += diag_block(m["n"], m["Sb"], m["Sbb"])
                g[j] += gj
        Ep = 0.0
        for f in free:
            if w > 0.0:
                Hd[f][:3, :3] += w * np.eye(3)
                dt = ts[f] - prior_t[f]
                g[f][:3] += w * (Rs[f].T @ dt)
                Ep += w * float(dt @ dt)
        return Hd, g, Hij, E, Ep

    def matvec(Hd, Hij, x):
        y = np.zeros_like(x)
        for f in free:
            acc = Hd[f] @ x[pos[f]]
            for (k, side) in adj[f]:
                i, j = pairs[k]
                other = j if side == 0 else i
                if other in pos:
                    acc = acc + (Hij[k] @ x[pos[other]] if side == 0 else Hij[k].T @ x[pos[other]])
            y[pos[f]] = acc
        return y

    def gnorm(g):
        return float(np.sqrt(sum(float(v @ v) for v in g.values()))) if g else 0.0

    last_step = 0.0
    for it in range(int(gn_iterations) + 1):
        Hd, g, Hij, E, Ep = assemble()
        if it == 0:
            out["e_before"], out["energy_before"], out["grad_before"] = E.copy(), float(E.sum() + Ep), gnorm(g)
        if it == int(gn_iterations) or not free or not edges:
            out["e_after"], out["energy_after"], out["grad_after"] = E.copy(), float(E.sum() + Ep), gnorm(g)
            break
        Minv = {f: invert6(Hd[f]) for f in free}
        for f in free:  # a block that is not positive definite: the frame stands still for this step
            if Minv[f] is None:
                out["flags"] |= FLAG_SINGULAR
                Minv[f] = np.zeros((6, 6))
        n = len(free)
        x = np.zeros((n, 6))
        r = -np.stack([g[f] for f in free])
        z = np.stack([Minv[f] @ r[pos[f]] for f in free])
        p = z.copy()
        rz = float((r * z).sum())
        for _ in range(int(cg_iterations)):
            Hp = matvec(Hd, Hij, p)
            pHp = float((p * Hp).sum())
            if not (pHp > 0.0) or not np.isfinite(pHp) or not np.isfinite(rz):
                out["flags"] |= FLAG_CG_STOPPED
                break
            alpha = rz / pHp
            x = x + alpha * p
            r = r - alpha * Hp
            z = np.stack([Minv[f] @ r[pos[f]] for f in free])
            rz_new = float((r * z).sum())
            beta = rz_new / rz
            if not np.isfinite(beta):
                out["flags"] |= FLAG_CG_STOPPED
                break
            p = z + beta * p
            rz = rz_new
        last_step = float(np.abs(x).max())
        for f in free:
            dx = x[pos[f]]
            ts[f] = ts[f] + Rs[f] @ dx[:3]
            Rs[f] = Rs[f] @ cayley(dx[3:])
    T = np.zeros((F, 12))
    pout = poses.copy()
    for f in range(F):
        if role[f] == FREE:
            T[f] = np.concatenate([Rs[f], ts[f][:, None]], 1).reshape(12)
            pout[f, :12] = T[f].astype(np.float32)
            pout[f, 12:] = (0, 0, 0, 1)
        else:
            T[f] = poses[f, :12].astype(np.float64)
    out.update(poses=pout, T=T, role=role, degree=degree, last_step=last_step, n_free=len(free),
               n_gauge=int(((role == FIXED) & (degree > 0)).sum()), n_floating=int((role == FLOATING).sum()),
               n_rejected=int((role == REJECTED).sum()), n_edges=len(edges), n_used_total=int(out["n_used"][out["edge"] != 0].sum()),
               Rs=Rs, ts=ts, free=free, pairs=pairs)
    return out


def state_of(T12):
    """[F, 12] fp64 poses -> (Rs, ts) as direct_energy takes them"""
    T = np.asarray(T12, np.float64).reshape(-1, 3, 4)
    return [t[:, :3] for t in T], [t[:, 3] for t in T]


# ---- worlds ---------------------------------------------------------------------------------------------------------------
def loop_poses(n, radius=None, step=0.5):
    """n true poses on a closed circle in the xz-plane, `step` metres apart, the camera turning with the path"""
    radius = step * n / (2.0 * np.pi) if radius is None else radius
    out = []
    for k in range(n):
        th = 2.0 * np.pi * k / n
        T = np.eye(4)
        T[:3, :3] = R.rot([0.1, 1.0, 0.05], 0.3 * np.sin(th))
        T[:3, 3] = (radius * np.cos(th), 0.05 * np.sin(3 * th), radius * np.sin(th))
        out.append(T)
    return np.stack(out)


def loop_pairs(prior, dist_nearby, range_width=8):
    """the chain's static list plus nothing: on a closed loop the last frames are near the first, so the list closes it"""
    return R.pair_list(prior, dist_nearby, range_width)
