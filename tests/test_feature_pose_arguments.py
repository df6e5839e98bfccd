"""GPU test of the checks the seven feature-pose entry points share (o3dr_match_knn2_hamming, o3dr_keypoints_3d,
o3dr_estimate_rigid_transform, o3dr_ransac_rigid, o3dr_pose_chain, o3dr_pose_chain_robust, o3dr_pose_graph_refine): one
table of the bad arguments they have in common, at the raw ctypes level, in the pattern of test_image_stack_arguments.py.
Every rejection is checked for its code, its o3dr_last_error() text, for the host outputs the operator's rule zeroes (they
start from a 0x5A fill) and for having launched nothing; a good call of the same operator follows, on a 2-frame pool of
70 + 5 rows, whose outputs are held to the operator's Python reference.  Two bad arguments at once pin which check comes
first.  The texts are literals."""
import ctypes as C
import functools

import numpy as np
import pytest

import pose_chain_reference as PC
import pose_graph_reference as PG
import ransac_rigid_reference as RR

pytestmark = pytest.mark.gpu

SIZES = (70, 5)
N = sum(SIZES)
FILL = 0x5A
THR, ITER, SEED = 0.05, 32, 99
NAN = float("nan")


def filled(shape, dtype):
    a = np.zeros(shape, dtype)
    a.view(np.uint8).reshape(-1)[:] = FILL
    return a


def is_zero(a):
    return not np.asarray(a).view(np.uint8).any()


def is_fill(a):
    return bool((np.asarray(a).view(np.uint8) == FILL).all())


def staged(a, mem):
    """an output the call stages as host memory: zeroed on an error when mem says host, untouched when mem is no kind at all"""
    return is_zero(a) if mem == 0 else is_fill(a)


def ptr(a):
    return None if a is None else a.ctypes.data


@functools.lru_cache(maxsize=None)
def world():
    """frame 0: 70 landmarks; frame 1: 5 of them.  kp3 exact up to rounding, one gross outlier in frame 1"""
    rng = np.random.default_rng(5)
    w = PC.make_world(5, [np.arange(70), rng.choice(70, 5, replace=False)], 70, step=0.1, prior_err=0.01)
    w["kp3"] = w["kp3"].copy()
    w["kp3"][72] += np.float32(2.0)
    w["points"] = PC.points(w["kp3"])
    w["pairs"] = np.array([[1, 0]], np.int32)
    return w


class Op:
    ransac = False

    def defaults(self):
        return dict(mem=0)

    def run(self, L, lib, h, change):
        a = {**self.defaults(), **change}
        return self.call(L, lib, h, a), a


class Match(Op):
    name, off_name, null_text = "match_knn2_hamming", "desc_offsets", "desc is NULL"

    def __init__(self, L):
        self.kinds = (L.K_MATCH,)
        w = world()
        idx, dist = PC.knn2_ref(w["desc"][70:], w["desc"][:70])
        self.ref = (idx, dist, PC.good_ref(dist))

    def defaults(self):
        w = world()
        return dict(mem=0, desc=w["desc"], off=w["offsets"], ratio=0.5, max_distance=40)

    def call(self, L, lib, h, a):
        out, good, n = filled(8, L.KNN2), filled(8, np.uint8), C.c_int64(0x5A5A)
        prs = world()["pairs"]
        rc = lib.o3dr_match_knn2_hamming(h, ptr(a["desc"]), ptr(a["off"]), 2, ptr(prs), 1, C.byref(L.MatchParamsStruct(a["ratio"], a["max_distance"])),
                                         ptr(out), ptr(good), 8, C.byref(n), a["mem"])
        return rc, dict(out=out, good=good, n=n.value)

    def zeroed(self, o, a):
        return o["n"] == 0 and staged(o["out"], a["mem"]) and staged(o["good"], a["mem"])

    def check(self, L, o):
        assert o["n"] == 5
        assert np.array_equal(o["out"]["train_idx"][:5], self.ref[0]) and np.array_equal(o["out"]["distance"][:5], self.ref[1])
        assert np.array_equal(o["good"][:5] != 0, self.ref[2]) and (o["good"][5:] == FILL).all()


class Keypoints(Op):
    name, off_name, null_text = "keypoints_3d", "kp_offsets", None

    def __init__(self, L, orc, Q, frames):
        self.kinds = (L.K_OTHER,)
        self.disp = np.ascontiguousarray(np.stack([f[0] for f in frames]))
        rows, cols = self.disp.shape[1:]
        rng = np.random.default_rng(3)
        self.kp = np.stack([rng.uniform(0, cols, N), rng.uniform(0, rows, N)], 1).astype(np.float32)
        self.off = np.array([0, 70, 75], np.int64)
        ref = np.zeros(N, L.POINT)
        for k in ("x", "y", "z"):
            ref[k] = np.nan
        for f in range(2):
            sl = slice(int(self.off[f]), int(self.off[f + 1]))
            x, y = np.trunc(self.kp[sl, 0]).astype(int), np.trunc(self.kp[sl, 1]).astype(int)
            ok = (x >= int(cols / 8)) & (x < cols - 20) & (y >= 20) & (y < rows - 20)
            ok[ok] = self.disp[f][y[ok], x[ok]] > 64.0
            pts = orc.create_single_img_pt_cloud(self.disp[f], frames[f][1], Q, jump_pixels=0, kp_xy=self.kp[sl])
            assert len(pts) == int(ok.sum()) > 0
            for k in ("x", "y", "z"):
                ref[k][np.nonzero(ok)[0] + sl.start] = pts[k]
        self.ref = ref

    def defaults(self):
        return dict(mem=0, off=self.off)

    def call(self, L, lib, h, a):
        out, n = filled(N, L.POINT), C.c_int64(0x5A5A)
        rows, cols = self.disp.shape[1:]
        rc = lib.o3dr_keypoints_3d(h, ptr(self.disp), rows * cols, cols, None, 0, 0, rows, cols, None, 2, ptr(self.kp), ptr(a["off"]),
                                   ptr(out), N, C.byref(n), a["mem"])
        return rc, dict(out=out, n=n.value)

    def zeroed(self, o, a):
        return o["n"] == 0 and staged(o["out"], a["mem"])

    def check(self, L, o):
        assert o["n"] == N and (o["out"]["rgba"] == 0).all()
        for k in ("x", "y", "z"):
            fin = np.isfinite(self.ref[k])
            assert np.array_equal(np.isnan(o["out"][k]), ~fin) and np.array_equal(o["out"][k][fin].view(np.uint32), self.ref[k][fin].view(np.uint32))


def _pairs_case():
    rng = np.random.default_rng(17)
    src = rng.uniform(-3, 3, (N, 3)).astype(np.float32)
    tgt = (src.astype(np.float64) @ PC.rot([0.3, 1.0, -0.2], 0.4).T + np.array([0.5, -1.0, 2.0])).astype(np.float32)
    tgt[[3, 40, 72]] += np.float32(1.5)  # outliers
    src[10, 1] = np.nan
    return src, tgt


class Rigid(Op):
    name = "estimate_rigid_transform"

    def __init__(self, L):
        self.kinds = (L.K_OTHER,)
        self.src, self.tgt = _pairs_case()
        self.psrc, self.ptgt = PC.points(self.src), PC.points(self.tgt)
        self.seg = np.array([0, 70, 75], np.int64)
        self.mask = np.ones(N, np.uint8)
        self.mask[[3, 40, 72]] = 0

    def defaults(self):
        return dict(mem=0, seg=self.seg, n_segs=2)

    def call(self, L, lib, h, a):
        res = filled(2, L.RIGID_RESULT)
        rc = lib.o3dr_estimate_rigid_transform(h, ptr(self.psrc), ptr(self.ptgt), N, ptr(a["seg"]), a["n_segs"],
                                               ptr(self.mask), ptr(res), a["mem"])
        return rc, dict(res=res)

    def zeroed(self, o, a):
        z = max(a["n_segs"], 0)
        return is_zero(o["res"][:z]) and is_fill(o["res"][z:])

    def check(self, L, o):
        for s in range(2):
            use = np.zeros(N, bool)
            use[self.seg[s]:self.seg[s + 1]] = True
            use &= (self.mask != 0) & np.isfinite(self.src).all(1) & np.isfinite(self.tgt).all(1)
            r = o["res"][s]
            assert r["status"] == L.RIGID_OK and r["n_used"] == use.sum()
            assert np.abs(r["T"].reshape(4, 4) - PC.kabsch_rank_ref(self.src[use], self.tgt[use])).max() < 1e-9


class Ransac(Op):
    name, ransac = "ransac_rigid", True

    def __init__(self, L):
        self.kinds = (L.K_RANSAC,)
        self.src, self.tgt = _pairs_case()
        self.psrc, self.ptgt = PC.points(self.src), PC.points(self.tgt)
        self.seg = np.array([0, 70, 75], np.int64)
        self.ref = RR.ransac_ref(self.src, self.tgt, THR, ITER, SEED, seg_offsets=self.seg)

    def defaults(self):
        return dict(mem=0, seg=self.seg, n_segs=2, threshold=THR, iterations=ITER)

    def call(self, L, lib, h, a):
        res, inl = filled(2, L.RANSAC_RESULT), filled(N, np.uint8)
        rc = lib.o3dr_ransac_rigid(h, ptr(self.psrc), ptr(self.ptgt), N, ptr(a["seg"]), a["n_segs"], None, None,
                                   C.byref(L.RansacParamsStruct(a["threshold"], SEED, a["iterations"], 0)), ptr(inl), ptr(res), a["mem"])
        return rc, dict(res=res, inl=inl)

    def zeroed(self, o, a):
        z = max(a["n_segs"], 0)
        return staged(o["inl"], a["mem"]) and is_zero(o["res"][:z]) and is_fill(o["res"][z:])

    def check(self, L, o):
        assert np.array_equal(o["inl"] != 0, self.ref["inlier"])
        for f in ("n_candidates", "n_inliers", "best_hypothesis", "status"):
            assert o["res"][f].tolist() == self.ref[f].tolist(), f
        assert o["res"]["sample"].tolist() == self.ref["sample"].tolist()
        assert np.abs(o["res"]["T"] - self.ref["T"]).max() <= 1e-9


class Chain(Op):
    name, off_name, null_text, robust = "pose_chain", "offsets", "desc / kp3 is NULL", False

    def __init__(self, L):
        self.kinds = (L.K_MATCH, L.K_POSE_CHAIN)
        w = world()
        kw = dict(min_matches=3)
        if self.robust:
            kw.update(ransac_threshold=THR, ransac_iterations=ITER, ransac_seed=SEED)
        self.ref = RR.robust_chain_ref(w["desc"], w["offsets"], w["kp3"], w["prior"], **kw)
        assert self.ref["status"].tolist() == [PC.ANCHOR, PC.MATCHED]

    def defaults(self):
        w = world()
        return dict(mem=0, desc=w["desc"], off=w["offsets"], ratio=0.5, max_distance=40, n_fixed=0, status=None, threshold=THR,
                    iterations=ITER)

    def call(self, L, lib, h, a):
        w = world()
        poses, frames, prs, n = filled((2, 16), np.float32), filled(2, L.CHAIN_FRAME), filled((2, 2), np.int32), C.c_int64(0x5A5A)
        rres = filled(2, L.RANSAC_RESULT)
        prm = L.ChainParamsStruct(2.0, float("inf"), 8, 3, a["ratio"], a["max_distance"])
        args = (h, ptr(a["desc"]), ptr(a["off"]), ptr(w["points"]), ptr(w["prior"]), 2, a["n_fixed"], ptr(w["prior"]) if a["n_fixed"] else None,
                ptr(a["status"]), C.byref(prm), ptr(poses), ptr(frames), ptr(prs), 2, C.byref(n), a["mem"])
        if self.robust:
            rc = lib.o3dr_pose_chain_robust(*args, C.byref(L.RansacParamsStruct(a["threshold"], SEED, a["iterations"], 0)), ptr(rres))
        else:
            rc = lib.o3dr_pose_chain(*args)
        return rc, dict(poses=poses, frames=frames, prs=prs, n=n.value, rres=rres)

    def zeroed(self, o, a):
        # (ransac_out is not zeroed: its length is an output)
        return o["n"] == 0 and staged(o["poses"], a["mem"]) and is_zero(o["frames"]) and is_zero(o["prs"]) and is_fill(o["rres"])

    def check(self, L, o):
        ref = self.ref
        assert o["n"] == 1 and o["prs"][0].tolist() == [1, 0]
        for f in ("status", "n_pairs", "n_pairs_accepted", "n_good", "n_used"):
            assert o["frames"][f].tolist() == ref[f].tolist(), f
        assert np.abs(o["frames"]["T"] - ref["T"]).max() < 1e-9 and np.abs(o["poses"] - ref["poses"]).max() < 1e-5
        if self.robust:
            RR.assert_ransac_equal(o["rres"][:1], ref)
            assert (o["rres"][1:].view(np.uint8) == FILL).all()


class ChainRobust(Chain):
    name, robust, ransac = "pose_chain_robust", True, True

    def __init__(self, L):
        super().__init__(L)
        self.kinds = (L.K_MATCH, L.K_RANSAC, L.K_POSE_CHAIN)


class Graph(Op):
    name, off_name, null_text, ransac = "pose_graph_refine", "offsets", "desc / kp3 is NULL", True

    def __init__(self, L):
        self.kinds = (L.K_MATCH, L.K_RANSAC, L.K_GRAPH_MOMENTS, L.K_GRAPH_SOLVE)
        w = world()
        ch = RR.robust_chain_ref(w["desc"], w["offsets"], w["kp3"], w["prior"], min_matches=3, ransac_threshold=THR,
                                 ransac_iterations=ITER, ransac_seed=SEED)
        self.status = np.array([PC.ANCHOR, PC.MATCHED], np.int32)
        self.ref = PG.refine_ref(w["desc"], w["offsets"], w["kp3"], w["prior"], self.status, w["pairs"], match=ch["match"], inlier=ch["inlier"])

    def defaults(self):
        w = world()
        return dict(mem=0, desc=w["desc"], off=w["offsets"], ratio=0.5, max_distance=40, status=self.status, threshold=THR, iterations=ITER)

    def call(self, L, lib, h, a):
        w = world()
        poses, frames, edges = filled((2, 16), np.float32), filled(2, L.REFINE_FRAME), filled(1, L.REFINE_EDGE)
        res = L.RefineResultStruct()
        C.memset(C.byref(res), FILL, C.sizeof(res))
        prm = L.RefineParamsStruct(0.0, 5, 32, 3, a["ratio"], a["max_distance"], 0)
        rc = lib.o3dr_pose_graph_refine(h, ptr(a["desc"]), ptr(a["off"]), ptr(w["points"]), 2, ptr(w["prior"]), ptr(a["status"]), None, None,
                                        ptr(w["pairs"]), 1, C.byref(prm), C.byref(L.RansacParamsStruct(a["threshold"], SEED, a["iterations"], 0)),
                                        ptr(poses), ptr(frames), ptr(edges), C.byref(res), a["mem"])
        return rc, dict(poses=poses, frames=frames, edges=edges, res=res)

    def zeroed(self, o, a):
        return staged(o["poses"], a["mem"]) and is_zero(o["frames"]) and is_zero(o["edges"]) and not any(bytes(o["res"]))

    def check(self, L, o):
        ref, res = self.ref, o["res"]
        assert o["frames"]["role"].tolist() == ref["role"].tolist() and o["frames"]["degree"].tolist() == ref["degree"].tolist()
        assert o["edges"]["n_good"].tolist() == ref["n_good"].tolist() and o["edges"]["n_used"].tolist() == ref["n_used"].tolist()
        assert o["edges"]["edge"].tolist() == ref["edge"].tolist()
        assert (res.n_free, res.n_gauge, res.n_edges, res.n_used) == (ref["n_free"], ref["n_gauge"], ref["n_edges"], ref["n_used_total"])
        assert abs(res.energy_before - ref["energy_before"]) <= 1e-9 * ref["energy_before"]
        assert np.abs(o["poses"] - ref["poses"]).max() < 1e-5


def bad_arguments(op):
    """(what, the changed arguments, the code's text today) for the arguments this operator has"""
    d = op.defaults()
    rows = [("mem = 2", dict(mem=2), "bad mem kind")]
    if "off" in d:
        o = d["off"]
        rows += [("offsets[0] < 0", dict(off=np.array([-1, 70, 75], np.int64)), f"{op.off_name}[0] must be >= 0"),
                 ("decreasing offsets", dict(off=np.array([o[0], 70, 69], np.int64)), f"{op.off_name} must not decrease")]
    if "desc" in d:
        rows += [("NULL pool with rows", dict(desc=None), op.null_text)]
    if "ratio" in d:
        rows += [("ratio = 0", dict(ratio=0.0), "ratio must be finite and > 0"),
                 ("ratio = nan", dict(ratio=NAN), "ratio must be finite and > 0"),
                 ("max_distance = 258", dict(max_distance=258), "max_distance must be in [0, 257]")]
    if "status" in d:
        rows += [("a status_in value of 5", dict(status=np.array([5, 1], np.int32), n_fixed=1), "status_in holds a value outside O3DR_CHAIN_*")]
    if "n_segs" in d:
        rows += [("n_segs = 0", dict(n_segs=0), "n_segs must be >= 1"),
                 ("NULL seg_offsets with n_segs = 2", dict(seg=None), "seg_offsets is NULL with n_segs != 1"),
                 ("decreasing seg_offsets", dict(seg=np.array([0, 70, 69], np.int64)), "seg_offsets must not decrease and stay within [0, n]"),
                 ("seg_offsets past n", dict(seg=np.array([0, 70, 76], np.int64)), "seg_offsets must not decrease and stay within [0, n]")]
    if op.ransac:
        rows += [("RANSAC threshold = 0", dict(threshold=0.0), "the RANSAC threshold must be finite and > 0"),
                 ("RANSAC iterations = 0", dict(iterations=0), "RANSAC iterations must be in [1, 65536]"),
                 ("RANSAC iterations = 65537", dict(iterations=65537), "RANSAC iterations must be in [1, 65536]")]
    return rows


# two bad arguments at once: the text of the check that comes first
ORDER = {
    "match_knn2_hamming": [(dict(mem=2, ratio=0.0), "bad mem kind"), (dict(ratio=0.0, off=np.array([-1, 70, 75], np.int64)), "ratio must be finite and > 0")],
    "keypoints_3d": [(dict(mem=2, off=np.array([-1, 70, 75], np.int64)), "bad mem kind")],
    "estimate_rigid_transform": [(dict(mem=2, n_segs=0), "bad mem kind"), (dict(n_segs=0, seg=None), "n_segs must be >= 1")],
    "ransac_rigid": [(dict(mem=2, n_segs=0), "bad mem kind"), (dict(n_segs=0, threshold=0.0), "n_segs must be >= 1"),
                     (dict(threshold=0.0, seg=np.array([0, 70, 76], np.int64)), "the RANSAC threshold must be finite and > 0")],
    "pose_chain": [(dict(mem=2, ratio=0.0), "bad mem kind"), (dict(ratio=0.0, off=np.array([-1, 70, 75], np.int64)), "ratio must be finite and > 0"),
                   (dict(off=np.array([-1, 70, 75], np.int64), desc=None), "offsets[0] must be >= 0")],
    "pose_chain_robust": [(dict(mem=2, threshold=0.0), "bad mem kind"), (dict(threshold=0.0, ratio=0.0), "the RANSAC threshold must be finite and > 0")],
    "pose_graph_refine": [(dict(mem=2, ratio=0.0), "bad mem kind"), (dict(threshold=0.0, ratio=0.0), "the RANSAC threshold must be finite and > 0"),
                          (dict(desc=None, status=np.array([5, 1], np.int32)), "desc / kp3 is NULL")],
}


def test_shared_bad_arguments_then_good_calls(orc, Q, frame_1248, frame_1249):
    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import _lib as L
    lib = L.load_library()
    ops = (Match(L), Keypoints(L, orc, Q, (frame_1248, frame_1249)), Rigid(L), Ransac(L), Chain(L), ChainRobust(L), Graph(L))
    every_kind = range(len(L.KERNEL_NAMES))
    with o3dr.Context(0, Q=Q) as ctx:
        def good(op, what):
            (rc, out), _ = op.run(L, lib, ctx._h, {})
            assert rc == 0, f"{op.name}, {what}: {lib.o3dr_last_error().decode()}"
            op.check(L, out)

        def rejected(op, what, change, text):
            ctx.profileReset()
            (rc, out), a = op.run(L, lib, ctx._h, change)
            assert rc == L.ERR_INVALID_ARG, f"{op.name}, {what}: returned {rc}"
            assert lib.o3dr_last_error().decode() == text, f"{op.name}, {what}: {lib.o3dr_last_error().decode()!r}"
            assert op.zeroed(out, a), f"{op.name}, {what}: the host outputs are not zeroed by the operator's rule"
            assert all(ctx.profileRead(k)[1] == 0 for k in every_kind), f"{op.name}, {what}: a rejected call launched a kernel"

        ctx.profileEnable(-1, True)
        try:
            for op in ops:
                good(op, "the first call")
                for what, change, text in bad_arguments(op):
                    rejected(op, what, change, text)
                    good(op, f"after {what}")
                    assert any(ctx.profileRead(k)[1] > 0 for k in op.kinds), f"{op.name}: the good call launched nothing"
                for change, text in ORDER[op.name]:
                    rejected(op, f"{sorted(change)} at once", change, text)
                good(op, "after the pairs of bad arguments")
        finally:
            ctx.profileEnable(-1, False)
            ctx.profileReset()
