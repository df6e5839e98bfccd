"""What the Python binding hands to the library, recorded without the library: a fake libo3dr that records every call, and
the cases test_binding_calls.py replays against tests/golden/binding_calls.json.

The fake (FakeLib) stands in for _lib.load_library()'s result.  Every o3dr_* attribute is a function that records its
arguments and returns 0.  A result struct passed by reference (a class named *ResultStruct, or the per-frame *InfoStruct
arrays of the image operators) is filled with distinct values, field k getting k + 1 and array elements counted on (through
nested structs and through the frames of an info array); a by-reference counter gets 3 (COUNTERS overrides it per symbol:
matchDescriptors asserts the count it is given); a ctypes array passed as it is gets 1, 2, ...; *_default_params structs
stay untouched.  The handle o3dr_ctx_create writes is HANDLE.

A record holds, per library call: the symbol, every scalar by value, every struct passed by reference as a dict of its
fields on entry, and every pointer as one of
  "null/empty"  NULL, or the address of an input or returned array of zero elements (the library dereferences neither),
  "input k"     the address of the k-th array of the case's arguments (arguments first, keywords after, lists in order),
  "output k"    the address of the k-th array of the returned value, with its shape and dtype,
  "other"       any other non-null pointer;
and of the method's return value each element's type, shape and dtype, and each dataclass's repr.  Calls and return
values are written as one line of text each, e.g. `o3dr_transform_pt_cloud(other, in0, 7, in1, out0:POINT[7], 0)`: a struct
as Name{field=value,...} ({0}: every field zero), a counter as &value, a record dtype by its name in _lib.  The golden
file holds every distinct line once ("calls", "returns") and per case the indices of its lines.

    python tests/binding_call_cases.py --write [--root DIR]
writes the golden file from the package under DIR (default: this repository).  The file in git was written from the
api.py of the commit before the binding's intakes, allocator and result path were unified, and is kept unchanged: the
binding must keep making the same calls."""
import ctypes as C
import dataclasses
import inspect
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "binding_calls.json")
HANDLE = 0x1000
COUNTERS = {"o3dr_match_knn2_hamming": 5}  # the 5 query rows of the pool's pair (1, 0)
# the per-frame info arrays reach the library as a bare address: symbol -> (argument index, struct name, index of F)
INFO_ARRAYS = {"o3dr_disparity_filter": (11, "DisparityFilterInfoStruct", 6), "o3dr_multiview_filter": (14, "MultiviewInfoStruct", 6),
               "o3dr_multiview_fuse": (15, "MultiviewFuseInfoStruct", 6), "o3dr_segment_image": (11, "SegmentInfoStruct", 6)}


class Pointer(int):
    """an address among a call's recorded arguments, until resolve() names it"""


def _fill(obj, k=0):
    for name, _ in obj._fields_:
        v = getattr(obj, name)
        if isinstance(v, C.Structure):
            k = _fill(v, k)
        elif isinstance(v, C.Array):
            for i in range(len(v)):
                k += 1
                v[i] = k
        else:
            k += 1
            setattr(obj, name, k)
    return k


def _fields(obj):
    out = {}
    for name, tp in obj._fields_:
        v = getattr(obj, name)
        if isinstance(v, C.Structure):
            out[name] = _fields(v)
        elif isinstance(v, C.Array):
            out[name] = list(v)
        elif tp is C.c_void_p:
            out[name] = Pointer(v or 0)
        else:
            out[name] = v
    return out


class FakeLib:
    def __init__(self, L):
        self.L = L
        self.argtypes = {name: args for name, _, args in L.SYMBOLS}
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("o3dr_"):
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def _call(self, name, args):
        types = self.argtypes[name]
        assert len(args) == len(types), f"{name}: {len(args)} arguments for {len(types)}"
        rec = []
        for a, tp in zip(args, types):
            obj = getattr(a, "_obj", None)  # what C.byref() holds
            if obj is not None and isinstance(obj, C.Structure):
                rec.append({"struct": type(obj).__name__, "fields": _fields(obj)})
                if type(obj).__name__.endswith("ResultStruct") and not name.endswith("_default_params"):
                    _fill(obj)
            elif obj is not None:  # a by-reference counter, or the handle
                rec.append({"counter": obj.value or 0})
                obj.value = HANDLE if name == "o3dr_ctx_create" else COUNTERS.get(name, 3)
            elif isinstance(a, C.Array):
                rec.append({"array": list(a)})
                for i in range(len(a)):
                    a[i] = i + 1
            elif tp is C.c_void_p or isinstance(a, C.c_void_p) or a is None:
                rec.append(Pointer((a.value if isinstance(a, C.c_void_p) else a) or 0))
            else:
                rec.append(a)
        if name in INFO_ARRAYS:
            at, struct, f_at = INFO_ARRAYS[name]
            if rec[at]:
                k = 0
                for s in (getattr(self.L, struct) * int(args[f_at])).from_address(int(rec[at])):
                    k = _fill(s, k)
        self.calls.append({"symbol": name, "args": rec})
        return 0


def _is_array(x):
    return isinstance(x, np.ndarray) or type(x).__module__.startswith("torch")


def _address(x):
    return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()


def _count(x):
    return x.size if isinstance(x, np.ndarray) else x.numel()


def _arrays(x):
    """the arrays of a case's arguments or of a returned value, in order"""
    if _is_array(x):
        return [x]
    if isinstance(x, (list, tuple)):
        return [a for v in x for a in _arrays(v)]
    if isinstance(x, dict):
        return [a for v in x.values() for a in _arrays(v)]
    return []


def _dtype(x):
    """an array's dtype, a record dtype by its name in _lib"""
    from online_3d_reconstruction_amd import _lib as L
    names = {str(v): k for k, v in vars(L).items() if isinstance(v, np.dtype)}
    return names.get(str(x.dtype), str(x.dtype).replace("torch.", ""))


def _typed(x):
    return f"{_dtype(x)}{[int(v) for v in x.shape]}".replace(" ", "")


def _describe(x):
    """a returned value as text"""
    if _is_array(x):
        return f"{type(x).__name__}:{_typed(x)}"
    if dataclasses.is_dataclass(x):
        return repr(x)
    if isinstance(x, (list, tuple)):
        body = ", ".join(_describe(v) for v in x)
        return f"[{body}]" if isinstance(x, list) else f"({body})"
    return f"{type(x).__name__}:{x!r}"


def resolve(calls, inputs, returned):
    """the recorded calls as text, every Pointer named"""
    outs = returned if isinstance(returned, tuple) else (returned,)
    names = {}
    for k, x in reversed(list(enumerate(outs))):
        if _is_array(x):
            names[_address(x)] = "null" if _count(x) == 0 else f"out{k}:{_typed(x)}"
    for k, x in reversed(list(enumerate(inputs))):
        names[_address(x)] = "null" if _count(x) == 0 else f"in{k}"
    names[0] = "null"

    def zero(v):
        return all(zero(x) for x in v.values()) if isinstance(v, dict) else all(zero(x) for x in v) if isinstance(v, list) else \
            not isinstance(v, Pointer) and v == 0

    def text(v):
        if isinstance(v, Pointer):
            return names.get(int(v), "other")
        if isinstance(v, dict) and "struct" in v:
            return v["struct"] + ("{0}" if zero(v["fields"]) else text(v["fields"]))
        if isinstance(v, dict) and "counter" in v:
            return f"&{v['counter']}"
        if isinstance(v, dict) and "array" in v:
            return "array" + text(v["array"])
        if isinstance(v, dict):
            return "{" + ",".join(f"{k}={text(x)}" for k, x in v.items()) + "}"
        if isinstance(v, list):
            return "[" + ",".join(text(x) for x in v) + "]"
        return repr(v.item() if isinstance(v, np.generic) else v)
    return [f"{c['symbol']}({', '.join(text(a) for a in c['args'])})" for c in calls]


# -- inputs -------------------------------------------------------------------------------------------------------------
def cloud(n, seed=0):
    from online_3d_reconstruction_amd import POINT
    rng = np.random.default_rng(100 + seed)
    p = np.zeros(n, POINT)
    for k, ax in enumerate("xyz"):
        p[ax] = ((3.0, 3.0, 0.5)[k] * rng.random(n)).astype(np.float32)
    p["rgba"] = rng.integers(0, 1 << 24, n, dtype=np.uint32)
    return p


def raster(H, W):
    r = (np.arange(H * W, dtype=np.float32).reshape(H, W) * np.float32(0.07)).copy()
    if r.size:
        r[1, 2] = np.nan
    return r


def pool():
    """the 2-frame pool of 70 + 5 rows of test_feature_pose_arguments.py"""
    import pose_chain_reference as PC
    rng = np.random.default_rng(5)
    w = PC.make_world(5, [np.arange(70), rng.choice(70, 5, replace=False)], 70, step=0.1, prior_err=0.01)
    w["kp3"] = w["kp3"].copy()
    w["kp3"][72] += np.float32(2.0)
    w["points"] = PC.points(w["kp3"])
    w["pairs"] = np.array([[1, 0]], np.int32)
    return w


def images(F=2, rows=8, cols=8, ch=1):
    rng = np.random.default_rng(9)
    return rng.integers(0, 256, (F, rows, cols) + ((3,) if ch == 3 else ()), dtype=np.uint8)


def as_kind(x, kind):
    """x as the case's input kind: itself, or a torch host tensor of the same bytes"""
    if kind == "numpy" or not isinstance(x, np.ndarray):
        return x
    import torch
    if x.dtype.names:  # POINT records: [n, 4] int32
        x = x.view(np.int32).reshape(-1, 4)
    return torch.from_numpy(np.ascontiguousarray(x))


def flags(method, on):
    """every return_* keyword of the method, all off or all on"""
    return {k: on for k in inspect.signature(method).parameters if k.startswith("return_")}


def cases(kinds=("numpy", "torch")):
    """-> [(id, method name, args, kwargs, flags on?)], the arrays already of the case's input kind"""
    out = []
    T = np.eye(4, dtype=np.float32)
    w = pool()

    def add(name, method, args, kwargs=None, kind_list=kinds, both=True):
        for kind in kind_list:
            for on in ((False, True) if both else (False,)):
                a = [as_kind(v, kind) if not isinstance(v, list) else [as_kind(u, kind) for u in v] for v in args]
                kw = {k: as_kind(v, kind) for k, v in (kwargs or {}).items()}
                out.append((f"{method}-{name}-{kind}-{'on' if on else 'off'}", method, a, kw, on))

    for n in (7, 1, 0):
        c = cloud(n)
        add(f"n{n}", "transformPtCloud", [c, T], both=False)
        add(f"n{n}", "downsamplePtCloud", [c, True])
        add(f"n{n}", "statisticalOutlierRemoval", [c], both=False)
        add(f"n{n}", "voxelGrid", [c, [0.2, 0.2, 0.2]], dict(min_points=2))
        add(f"n{n}", "mlsSmooth", [c, 0.6])
        add(f"n{n}", "segmentPlane", [c, 0.05], dict(max_iterations=64, seed=3))
        add(f"n{n}-tiles", "segmentPlane", [c, 0.05], dict(max_iterations=64, tile_size=1.5, seed=3, project=True))
        add(f"n{n}", "meshSurface", [c, 0.25, 1.0])
        add(f"n{n}", "rasterExtent", [c, 0.25], both=False)
        add(f"n{n}", "rasterizeMap", [c, 0.25])
        add(f"n{n}-box", "rasterizeMap", [c, 0.25], dict(bounds=(0, 0, 5, 4), select="top", fill_radius=2, light=(-1, 1, 1)))
        add(f"n{n}-nobox", "rasterizeMap", [c, 0.25], dict(bounds=(0, 0, 0, 0)))
        add(f"n{n}", "groundFilter", [c, 0.25], dict(max_window_radius=4))
        add(f"n{n}-box", "groundFilter", [c, 0.25], dict(bounds=(0, 0, 5, 4), max_window_radius=4, fill_radius=1))
        add(f"n{n}-interp", "groundFilter", [c, 0.25], dict(bounds=(0, 0, 5, 4), max_window_radius=4, interpolate=True),
            kind_list=("numpy",))
        add(f"n{n}", "clusterCloud", [c, 0.3], dict(min_size=2))
        add(f"n{n}", "sampleRaster", [c, raster(4, 5), 0.25, (0, 0, 5, 4)])
        add(f"n{n}-r0", "sampleRaster", [c, raster(0, 0), 0.25, (0, 0, 0, 0)])
        for m in (7, 0):
            t = cloud(m, 1)
            add(f"n{n}-m{m}", "nearestNeighbors", [c, t], dict(max_distance=0.5), both=False)
            add(f"n{n}-m{m}", "icpAlign", [c, t], both=False)
            add(f"n{n}-m{m}-init", "icpAlign", [c, t], dict(T_init=T, max_iterations=3), both=False)
        t = cloud(n, 1)
        add(f"n{n}", "estimateRigidTransform", [c, t], both=False)
        add(f"n{n}-segs", "estimateRigidTransform", [c, t], dict(seg_offsets=[0, n // 2, n], mask=np.ones(n, bool)), kind_list=("numpy",),
            both=False)
        add(f"n{n}", "ransacRigid", [c, t, 0.05], dict(iterations=32, seed=99), both=False)
        add(f"n{n}-segs", "ransacRigid", [c, t, 0.05], dict(iterations=32, seed=99, seg_offsets=[0, n // 2, n], mask=np.ones(n, np.uint8),
                                                          seg_keys=[5, 6]), kind_list=("numpy",), both=False)
    for H, W in ((4, 5), (0, 0)):
        add(f"{H}x{W}", "interpolateRaster", [raster(H, W)])
        add(f"{H}x{W}-level", "interpolateRaster", [raster(H, W)], dict(smooth=1, max_level=2))
        add(f"{H}x{W}", "contourRaster", [raster(H, W), 0.1])
        add(f"{H}x{W}-origin", "contourRaster", [raster(H, W), 0.1], dict(base=0.05, cell_size=0.25, origin=(3, -2)))

    # the feature methods, on the pool (and on an empty one)
    empty = dict(desc=np.zeros((0, 32), np.uint8), offsets=np.zeros(1, np.int64), points=cloud(0), prior=np.zeros((0, 16), np.float32))
    add("pool", "matchDescriptors", [w["desc"], w["offsets"], w["pairs"]], both=False)
    add("pool", "matchFeatures", [w["desc"][70:], w["desc"][:70], w["points"][70:], w["points"][:70]], kind_list=("numpy",), both=False)
    add("pool-ransac", "matchFeatures", [w["desc"][70:], w["desc"][:70], w["points"][70:], w["points"][:70]],
        dict(ransac_threshold=0.05, ransac_iterations=32, ransac_seed=99), kind_list=("numpy",), both=False)
    for name, p in (("pool", dict(desc=w["desc"], offsets=w["offsets"], points=w["points"], prior=w["prior"])), ("empty", empty)):
        F = len(p["offsets"]) - 1
        add(name, "poseChain", [p["desc"], p["offsets"], p["points"], p["prior"]], dict(min_matches=3))
        add(f"{name}-ransac", "poseChain", [p["desc"], p["offsets"], p["points"], p["prior"]],
            dict(min_matches=3, ransac_threshold=0.05, ransac_iterations=32, ransac_seed=99))
        add(f"{name}-refine", "poseChain", [p["desc"], p["offsets"], p["points"], p["prior"]], dict(min_matches=3, refine=True))
        add(name, "refinePoses", [p["desc"], p["offsets"], p["points"], p["prior"].reshape(F, 4, 4), np.ones(F, np.int32),
                                  w["pairs"][:F // 2]], dict(fixed=np.arange(F) == 0))
    add("history", "poseChain", [w["desc"], w["offsets"], w["points"], w["prior"]],
        dict(n_fixed=1, poses_in=w["prior"][:1], status_in=np.zeros(1, np.int32), min_matches=3))
    disp, bgr = images(2, 8, 8), images(2, 8, 8, 3)
    kp = [np.array([[1.5, 2.5], [3.0, 4.0], [6.0, 1.0]], np.float32), np.zeros((0, 2), np.float32)]
    add("single", "keypoints3D", [disp[0], kp[0]], kind_list=("numpy",), both=False)
    add("stack", "keypoints3D", [disp, kp], dict(poses=np.stack([T, T]), bgr=bgr), kind_list=("numpy",), both=False)
    add("none", "keypoints3D", [disp, [kp[1], kp[1]]], kind_list=("numpy",), both=False)

    # the frame entry points, the map of a camera, and the image operators (for the result path)
    for name, kw in (("plain", {}), ("kp", dict(kp_xy=kp[0]))):
        add(name, "createSingleImgPtCloud", [disp[0], bgr[0]], kw, both=False)
        add(name, "reprojectTransform", [disp[0], bgr[0], T], kw, both=False)
        add(name, "createAndTransformPtCloud", [disp[0], bgr[0], T], kw)
    K = np.array([[50.0, 0, 4], [0, 50.0, 4], [0, 0, 1]])
    add("host", "rectifyMaps", [K, np.zeros(5), np.eye(3), K, (4, 5)], kind_list=("numpy",), both=False)
    add("none", "rectifyMaps", [K, np.zeros(5), np.eye(3), K, (0, 0)], kind_list=("numpy",), both=False)
    poses = np.stack([T, T])
    add("stack", "findFeatures", [disp], dict(n_features=4, n_levels=2), kind_list=("numpy",))
    add("stack", "stereoDisparity", [disp, disp], dict(n_disparities=16), kind_list=("numpy",))
    add("subpixel", "stereoDisparity", [disp, disp], dict(n_disparities=16, subpixel=True), kind_list=("numpy",))
    add("stack", "filterDisparity", [disp], dict(median=3, max_speckle_size=4), kind_list=("numpy",))
    add("stack", "multiviewFilter", [disp, poses], dict(neighbors=np.array([[1], [0]], np.int32)), kind_list=("numpy",))
    add("nearby", "multiviewFilter", [disp, poses], dict(k=1), kind_list=("numpy",))
    add("stack", "multiviewFuse", [disp, poses], dict(neighbors=np.array([[1], [0]], np.int32)), kind_list=("numpy",))
    add("stack", "segmentImage", [bgr], dict(step=4), kind_list=("numpy",))
    add("valid", "rectify", [bgr, np.zeros((4, 5, 2), np.int32)], kind_list=("numpy",))
    return out


def run_case(o3dr, fake, case):
    """one case against a Context over the fake -> its record"""
    _, method, args, kwargs, on = case
    ctx = o3dr.Context(0)
    try:
        fn = getattr(ctx, method)
        fake.calls.clear()
        got = fn(*args, **kwargs, **flags(fn, on))
        calls = resolve(fake.calls, _arrays(args) + _arrays(kwargs), got)
    finally:
        ctx.close()
    return {"calls": calls, "returned": _describe(got)}


def install(patch):
    """the package with _lib.load_library replaced through patch(module, name, value) -> (package, fake)"""
    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import _lib as L
    fake = FakeLib(L)
    patch(L, "load_library", lambda: fake)
    return o3dr, fake


def load_golden():
    """the golden file -> {case id: its record}"""
    with open(GOLDEN) as f:
        g = json.load(f)
    return {k: {"calls": [g["calls"][c] for c in calls], "returned": g["returns"][ret]} for k, (calls, ret) in g["cases"].items()}


def first_difference(want, got):
    """a line on the first call of two records that differs, or on the returned values"""
    for k, (a, b) in enumerate(zip(want["calls"], got["calls"])):
        if a != b:
            return f"call {k} differs:\n  golden: {a}\n  now:    {b}"
    if len(want["calls"]) != len(got["calls"]):
        return f"{len(got['calls'])} calls for the golden file's {len(want['calls'])}:\n  golden: {want['calls']}\n  now:    {got['calls']}"
    return f"the returned value differs:\n  golden: {want['returned']}\n  now:    {got['returned']}"


def main(argv):
    root = argv[argv.index("--root") + 1] if "--root" in argv else os.path.dirname(HERE)
    sys.path.insert(0, root)
    o3dr, fake = install(setattr)
    records = {c[0]: run_case(o3dr, fake, c) for c in cases()}
    calls = sorted({c for r in records.values() for c in r["calls"]})
    returns = sorted({r["returned"] for r in records.values()})
    at = {c: k for k, c in enumerate(calls)}
    cs = {k: [[at[c] for c in r["calls"]], returns.index(r["returned"])] for k, r in records.items()}
    lines = lambda xs: "[\n" + ",\n".join(json.dumps(x) for x in xs) + "\n]"  # noqa: E731
    text = '{"calls": ' + lines(calls) + ',\n"returns": ' + lines(returns) + ',\n"cases": {\n' + \
        ",\n".join(", ".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in cs.items() if k.split("-")[0] == m)
                   for m in dict.fromkeys(k.split("-")[0] for k in cs)) + "\n}}\n"  # (one line per method)
    if "--write" in argv:
        with open(GOLDEN, "w") as f:
            f.write(text)
        print(f"{len(records)} cases from {o3dr.__file__} -> {GOLDEN}")
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main(sys.argv[1:])
