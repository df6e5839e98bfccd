"""GPU test of the front end the six image-stack operators share (o3dr_orb_detect, o3dr_rectify_remap, o3dr_stereo_disparity,
o3dr_disparity_filter, o3dr_multiview_filter, o3dr_segment_image): one table of the bad arguments they have in common.  Every
rejection is checked for its code, its o3dr_last_error() text and for having launched nothing, and is followed by a good call
of the same operator whose outputs equal the operator's Python reference.  The six good calls then run once more in reverse
order: whatever scratch the operators share, one operator's call leaves the next one's result unchanged.

All stacks are 2 frames of 9 x 33 pixels in host memory.  (At that size ORB's margin of 16 pixels leaves no keypoint: its
outputs are the counts, the offsets and the grey pyramid.)"""
import ctypes as C
import functools

import numpy as np
import pytest

import disparity_filter_reference as DF
import multiview_reference as MV
import orb_reference as ORB
import rectify_reference as RECT
import segment_reference as SEG
import stereo_reference as ST

pytestmark = pytest.mark.gpu

H, W, F = 9, 33, 2
SIDES = "rows and cols must be in 1..8192"


def _rng_images(channels, seed):
    shape = (F, H, W) + ((3,) if channels == 3 else ())
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


class Orb:
    name, px, null_text, sides_text = "orb_detect", 3, "img is NULL", SIDES
    prm = dict(n_features=64, scale_factor=1.3, n_levels=2, fast_threshold=20, edge=16, channels=3)

    def __init__(self, L):
        self.kinds = (L.K_ORB_PYRAMID, L.K_ORB_FAST, L.K_ORB_CANDIDATES, L.K_ORB_SELECT, L.K_ORB_DESCRIBE)
        self.img = _rng_images(3, 11)
        refs = [ORB.detect(f, 64, 1.3, 2, 20, 16) for f in self.img]
        self.n_levels_px = sum(lv.size for lv in refs[0]["levels"])
        counts = np.cumsum([0] + [len(r["kp"]) for r in refs])
        self.ref = (int(counts[-1]), counts.tolist(), np.concatenate([lv.ravel() for r in refs for lv in r["levels"]]))

    def call(self, L, lib, h, a):
        cap = F * 64
        kp, xy, desc = np.zeros(cap, L.ORB_KEYPOINT), np.zeros((cap, 2), np.float32), np.zeros((cap, 32), np.uint8)
        off, n, lev = np.zeros(F + 1, np.int64), C.c_int64(-1), np.full(F * self.n_levels_px, 0x5A, np.uint8)
        rc = lib.o3dr_orb_detect(h, a["ptr"](self.img), a["fs"], a["pitch"], a["rows"], a["cols"], a["n_frames"],
                                 C.byref(L.OrbParamsStruct(**self.prm)), kp.ctypes.data, xy.ctypes.data, desc.ctypes.data,
                                 off.ctypes.data, lev.ctypes.data, cap, C.byref(n), a["mem"])
        return rc, (int(n.value), off.tolist(), lev)


class Rectify:
    name, px, null_text = "rectify_remap", 1, "src / map / out is NULL"
    sides_text = "rows, cols, rows_out and cols_out must be in 1..8192"

    def __init__(self, L):
        self.kinds = (L.K_RECTIFY_MAPS, L.K_RECTIFY_REMAP)
        self.img = _rng_images(1, 12)
        # the identity calibration moved by a fraction of a pixel, at the source's own size: every tap interpolates
        case = dict(RECT.IDENTITY, K=RECT.K_ID + np.array([[0, 0, 0.3], [0, 0, -0.4], [0, 0, 0]]))
        self.maps = np.ascontiguousarray(RECT.maps_of(case, (H, W)))
        self.ref = RECT.rectify_remap_frames(self.img, self.maps, 7)

    def call(self, L, lib, h, a):
        out, valid = np.full((F, H, W), 0x5A, np.uint8), np.full((H, W), 0x5A, np.uint8)
        rc = lib.o3dr_rectify_remap(h, a["ptr"](self.img), a["fs"], a["pitch"], a["rows"], a["cols"], 1, a["n_frames"],
                                    self.maps.ctypes.data, H, W, 7, 0, out.ctypes.data, valid.ctypes.data, a["mem"])
        return rc, (out, valid)


class Stereo:
    name, px, null_text, sides_text = "stereo_disparity", 1, "left / right is NULL", SIDES
    prm = dict(n_disparities=32, min_disparity=0, p1=10, p2=120, n_paths=8, uniqueness=10, lr_max_diff=1, channels=1, group_frames=0)

    def __init__(self, L):
        self.kinds = (L.K_STEREO_CENSUS, L.K_STEREO_PATHS, L.K_STEREO_WINNER)
        self.right = _rng_images(1, 13)
        self.left = _rng_images(1, 14)
        self.left[:, :, 5:W - W // 4] = self.right[:, :, :W - W // 4 - 5]  # a known shift in the left part, noise elsewhere
        kw = {k: v for k, v in self.prm.items() if k not in ("channels", "group_frames")}
        self.ref = tuple(np.stack(o) for o in zip(*(ST.stereo_disparity(l, r, **kw) for l, r in zip(self.left, self.right))))

    def call(self, L, lib, h, a):
        disp = np.full((F, H, W), 0x5A, np.uint8)
        q4, cost, vol = (np.full((F, H, W) + t, 0x5A5A, np.uint16) for t in ((), (), (32,)))
        rc = lib.o3dr_stereo_disparity(h, a["ptr"](self.left), a["ptr"](self.right), a["fs"], a["pitch"], a["rows"], a["cols"],
                                       a["n_frames"], C.byref(L.StereoParamsStruct(**self.prm)), disp.ctypes.data, q4.ctypes.data,
                                       cost.ctypes.data, vol.ctypes.data, a["mem"])
        return rc, (disp, q4, cost, vol)


class DisparityFilter:
    name, px, null_text, sides_text = "disparity_filter", 1, "disp / out is NULL", SIDES

    def __init__(self, L):
        self.kinds = (L.K_DISP_MEDIAN, L.K_DISP_LABEL, L.K_DISP_SPECKLE)
        self.img = (np.random.RandomState(15).randint(0, 4, (F, H, W))).astype(np.uint8)
        out, labels, sizes, infos = DF.filter_frames(self.img, median_size=3, max_speckle_size=3, max_diff=0)
        self.ref = (out, labels, sizes, [tuple(getattr(i, k) for k, _ in L.DisparityFilterInfoStruct._fields_) for i in infos])

    def call(self, L, lib, h, a):
        out = np.full((F, H, W), 0x5A, np.uint8)
        labels, sizes = (np.full((F, H, W), 0x5A5A5A5A, np.int32) for _ in range(2))
        info = (L.DisparityFilterInfoStruct * F)()
        rc = lib.o3dr_disparity_filter(h, a["ptr"](self.img), a["fs"], a["pitch"], a["rows"], a["cols"], a["n_frames"],
                                       C.byref(L.DisparityFilterParamsStruct(1, 3, 3, 0, 0)), out.ctypes.data, labels.ctypes.data,
                                       sizes.ctypes.data, C.cast(info, C.c_void_p), a["mem"])
        return rc, (out, labels, sizes, [tuple(int(getattr(i, k)) for k, _ in L.DisparityFilterInfoStruct._fields_) for i in info])


class Multiview:
    name, px, null_text, sides_text = "multiview_filter", 1, "disp / out is NULL", SIDES

    def __init__(self, L):
        self.kinds = (L.K_MULTIVIEW,)
        self.img, self.Q, poses, _ = MV.plane_scene(H, W, F, 16, np.uint8, holes=0.1, max_shift=0.002)
        self.poses = np.ascontiguousarray(poses, np.float32)
        self.nb = np.ascontiguousarray(MV.nearby_frames(poses, 1), np.int32)
        out, support, violations, infos = MV.multiview_filter(self.img, self.Q, poses, self.nb, 0.5, 1, -1)
        self.ref = (out, support, violations, [tuple(int(v) for v in i) for i in infos])

    def call(self, L, lib, h, a):
        out, support, violations = (np.full((F, H, W), 0x5A, np.uint8) for _ in range(3))
        info = (L.MultiviewInfoStruct * F)()
        rc = lib.o3dr_multiview_filter(h, a["ptr"](self.img), a["fs"], a["pitch"], a["rows"], a["cols"], a["n_frames"],
                                       self.poses.ctypes.data, self.nb.ctypes.data, 1, C.byref(L.MultiviewParamsStruct(1, 0.5, 1, -1)),
                                       out.ctypes.data, support.ctypes.data, violations.ctypes.data, C.cast(info, C.c_void_p), a["mem"])
        return rc, (out, support, violations, [tuple(int(getattr(i, k)) for k, _ in L.MultiviewInfoStruct._fields_) for i in info])


class Segment:
    name, px, null_text, sides_text = "segment_image", 3, "img / labels is NULL", SIDES
    FIELDS = ("n_centres", "n_components", "n_merged", "n_labels", "largest", "smallest")

    def __init__(self, L):
        self.kinds = (L.K_SEG_ASSIGN, L.K_SEG_LABEL)
        self.img = np.stack([SEG.random_image(H, W, 3, seed=s) for s in (1, 2)])
        res = [SEG.segment(f, 4, 20, 2, None) for f in self.img]
        self.ref = tuple(np.stack([r[k] for r in res]) for k in ("labels", "raw", "sizes")) + ([tuple(r["info"][k] for k in self.FIELDS) for r in res],)

    def call(self, L, lib, h, a):
        labels = np.full((F, H, W), 0x5A5A5A5A, np.uint32)
        raw, sizes = (np.full((F, H, W), 0x5A5A5A5A, np.int32) for _ in range(2))
        info = (L.SegmentInfoStruct * F)()
        rc = lib.o3dr_segment_image(h, a["ptr"](self.img), a["fs"], a["pitch"], a["rows"], a["cols"], a["n_frames"],
                                    C.byref(L.SegmentParamsStruct(3, 4, 20, 2, -1, 0)), labels.ctypes.data, raw.ctypes.data,
                                    sizes.ctypes.data, C.cast(info, C.c_void_p), a["mem"])
        return rc, (labels, raw, sizes, [tuple(int(getattr(i, k)) for k in self.FIELDS) for i in info])


@functools.lru_cache(maxsize=None)
def operators():
    """the six operators with their inputs and references, computed once"""
    from online_3d_reconstruction_amd import _lib as L
    return tuple(cls(L) for cls in (Orb, Rectify, Stereo, DisparityFilter, Multiview, Segment))


def good_args(op):
    return dict(ptr=lambda x: x.ctypes.data, fs=H * W * op.px, pitch=W * op.px, rows=H, cols=W, n_frames=F, mem=0)


def bad_arguments(op):
    """(what, the changed arguments, today's o3dr_last_error() text), in the order the issue lists them"""
    return [("mem = 2", dict(mem=2), "bad mem kind"),
            ("n_frames = -1", dict(n_frames=-1), "bad frame count"),
            ("rows = 0", dict(rows=0), op.sides_text),
            ("cols = 8193", dict(cols=8193), op.sides_text),
            ("pitch one byte short", dict(pitch=W * op.px - 1), "pitch smaller than a row"),
            ("frame stride one byte short", dict(fs=H * W * op.px - 1), "frame stride smaller than a frame"),
            ("NULL input", dict(ptr=lambda x: None), op.null_text)]


def same(got, ref):
    return len(got) == len(ref) and all(np.array_equal(g, r) if isinstance(r, np.ndarray) else g == r for g, r in zip(got, ref))


def test_shared_bad_arguments_then_good_calls():
    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import _lib as L
    lib = L.load_library()
    ops = operators()
    every_kind = range(len(L.KERNEL_NAMES))
    with o3dr.Context(0, Q=next(op for op in ops if op.name == "multiview_filter").Q) as ctx:
        def good(op, what):
            rc, got = op.call(L, lib, ctx._h, good_args(op))
            assert rc == 0, f"{op.name}, {what}: {lib.o3dr_last_error().decode()}"
            assert same(got, op.ref), f"{op.name}, {what}: the outputs differ from the reference"

        ctx.profileEnable(-1, True)
        try:
            for op in ops:
                good(op, "the first call")
                for what, change, text in bad_arguments(op):
                    ctx.profileReset()
                    rc, _ = op.call(L, lib, ctx._h, {**good_args(op), **change})
                    assert rc == L.ERR_INVALID_ARG, f"{op.name}, {what}: returned {rc}"
                    assert lib.o3dr_last_error().decode() == text, f"{op.name}, {what}: {lib.o3dr_last_error().decode()!r}"
                    assert all(ctx.profileRead(k)[1] == 0 for k in every_kind), f"{op.name}, {what}: a rejected call launched a kernel"
                    good(op, f"after {what}")
                    assert any(ctx.profileRead(k)[1] > 0 for k in op.kinds), f"{op.name}: the good call launched nothing"
            for op in reversed(ops):
                good(op, "in reverse order")
        finally:
            ctx.profileEnable(-1, False)
            ctx.profileReset()
