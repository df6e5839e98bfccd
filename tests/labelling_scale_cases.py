"""The inputs and references of tests/test_labelling_scale.py, shared with the CPU tests that pin their conditions
(test_disparity_filter_reference.py, test_segment_reference.py).  255 x 1023 and its transpose are 16 x 16 = 256 tiles of
64 x 16 pixels with a remainder tile on both axes, 75 workgroups of border pairs and 1 019 of pixels, and 260 865 pixels:
past the single-workgroup scan of the segmentation's numbering.  Every image and every reference is computed once."""
import functools

import numpy as np

import disparity_filter_reference as D
import segment_reference as S
from test_disparity_filter import checkerboard, levels, unit

SIZES = [(255, 1023), (1023, 255)]
SIZE_IDS = [f"{h}x{w}" for h, w in SIZES]
TILE_X, TILE_Y = 64, 16

DF_WINDING = {
    "maze": lambda H, W: D.maze(H, W, 1),
    "spiral": D.spiral,
    "serpentine": D.serpentine,
    "serpentine transposed": lambda H, W: np.ascontiguousarray(D.serpentine(W, H).T),
    "comb": D.comb,
    "comb upside down": lambda H, W: np.ascontiguousarray(D.comb(H, W)[::-1]),
    "all equal": lambda H, W: np.full((H, W), 77, np.uint8),
    "checkerboard": checkerboard,
}
DF_ONE_COMPONENT = ("maze", "spiral", "serpentine", "serpentine transposed", "comb", "comb upside down", "all equal")
DF_OTHER = {
    "levels uint8": lambda H, W: levels(H, W, np.uint8, seed=H * 1000 + W),
    "levels uint16": lambda H, W: levels(H, W, np.uint16, seed=H * 1000 + W),
}


@functools.lru_cache(maxsize=None)
def df_input(name, H, W):
    img = (DF_WINDING.get(name) or DF_OTHER[name])(H, W)
    assert img.shape == (H, W)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def df_reference(name, H, W, median=0, size=100, diff=1):
    """-> out, labels, sizes, [Info] of tests/disparity_filter_reference.py"""
    out, labels, sizes, info = D.filter_disparity(df_input(name, H, W), median, size, diff)
    for a in (out, labels, sizes):
        a.setflags(write=False)
    return out, labels, sizes, [info]


# (median, max_diff in levels) of the many-component cases
DF_LEVEL_PARAMS = [(0, 0), (0, 1), (3, 0), (5, 1)]
DF_LEVEL_SPECKLE = 40


def df_level_diff(name, d):
    return d * unit(df_input(name, *SIZES[0]).dtype.type)


# ---- segmentation ----------------------------------------------------------------------------------------------------
def _bgr(grey):
    return np.ascontiguousarray(np.repeat(grey[:, :, None], 3, axis=2))


SEG_INPUTS = {
    "random bgr": lambda H, W: S.random_image(H, W, 3, seed=H * 1000 + W),
    "random grey": lambda H, W: S.random_image(H, W, 1, seed=H * 1000 + W),
    "maze": lambda H, W: S.maze(H, W, 1),
    "spiral": S.spiral,
    "checkerboard": S.checkerboard,
    "constant": S.constant_image,
    "maze bgr": lambda H, W: _bgr(S.maze(H, W, 1)),
    "checkerboard bgr": lambda H, W: _bgr(S.checkerboard(H, W)),
}


@functools.lru_cache(maxsize=None)
def seg_input(name, H, W):
    img = SEG_INPUTS[name](H, W)
    assert img.shape[:2] == (H, W)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def seg_reference(name, H, W, step, m, K, min_size):
    """-> labels, raw, sizes, [info] of tests/segment_reference.py"""
    r = S.segment(seg_input(name, H, W), step, m, K, min_size)
    for k in ("labels", "raw", "sizes"):
        r[k].setflags(write=False)
    return r["labels"], r["raw"], r["sizes"], [r["info"]]


# every segmentation the GPU tests ask for: (input, H, W, step, compactness, iterations, min_size)
SEG_RANDOM = [(f"random {c}", H, W, step, 20, 5, None) for c in ("bgr", "grey") for H, W in SIZES for step in (8, 16)]
SEG_WINDING = [(name, 255, 1023, 256, 0, K, min_size) for name in ("maze", "spiral") for K, min_size in ((1, 10000), (3, None), (0, 0))]
SEG_CHAIN = ("checkerboard", 255, 1023, 5, 0, 3, 10000)
SEG_CONSTANT = ("constant", 255, 1023, 8, 20, 3, None)
SEG_LARGE_Y = ("random grey", 8192, 9, 8, 20, 2, None)
SEG_STACK = [(name, 255, 1023, 16, 20, 5, None) for name in ("random bgr", "maze bgr", "checkerboard bgr")]
SEG_CASES = SEG_RANDOM + SEG_WINDING + [SEG_CHAIN, SEG_CONSTANT, SEG_LARGE_Y] + SEG_STACK[1:]


def seg_id(case):
    name, H, W, step, m, K, min_size = case
    return f"{name} {H}x{W} S {step} m {m} K {K} min_size {min_size}"


def tiles_of_largest_component(raw):
    """-> (pixels, tiles the pixels lie in) of the largest 4-connected component of equal raw labels"""
    H, W = raw.shape
    root = S.components(raw.astype(np.int64)).reshape(-1)
    count = np.bincount(root, minlength=H * W)
    sel = (root == int(count.argmax())).reshape(H, W)
    yy, xx = np.nonzero(sel)
    return int(count.max()), len(np.unique((yy // TILE_Y) * -(-W // TILE_X) + xx // TILE_X))
