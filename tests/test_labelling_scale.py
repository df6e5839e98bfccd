"""GPU tests of the two labelling operators, Context.filterDisparity and Context.segmentImage, on images of 256 tiles:
255 x 1023 and 1023 x 255 (tests/labelling_scale_cases.py).  Their union-find joins tiles through global memory with
atomic minima, so what can go wrong grows with the number of workgroups that pull at one tree: a link lost, a count added
twice or not at all, a root that is not the lowest index, a merge chain that ends at the wrong root.  Here a component
spans every tile, every phase has workgroups on every XCD, both axes end in a remainder tile and the segmentation's
numbering takes the chunked scan.  Every output and every info field is compared bit for bit with the numpy references;
each CPU-side condition a case rests on is asserted on the reference before the GPU is asked."""
import numpy as np
import pytest

import labelling_scale_cases as X
import test_disparity_filter as TD
import test_segment_image as TS

pytestmark = pytest.mark.gpu


# ---- disparity filter --------------------------------------------------------------------------------------------------
def winding_condition(name, H, W):
    img, ref = X.df_input(name, H, W), X.df_reference(name, H, W)
    info = ref[3][0]
    assert info.n_valid == int((img != 0).sum())
    if name in X.DF_ONE_COMPONENT:
        assert info.n_components == 1 and info.largest == info.n_valid and ref[1][img != 0].max() == 0
    if name == "all equal":
        assert info.largest == H * W
    if name == "checkerboard":
        assert info.n_components == info.n_valid == (H * W + 1) // 2 and info.n_removed == info.n_valid
    return img, ref


@pytest.mark.parametrize("H,W", X.SIZES, ids=X.SIZE_IDS)
@pytest.mark.parametrize("name", list(X.DF_WINDING))
def test_filter_winding_components(ctx, name, H, W):
    img, ref = winding_condition(name, H, W)
    TD.check(TD.run(ctx, img, 0, 100, 1), ref, f"{name} {H}x{W}")


def summed_size_condition(H, W):
    n_valid = int((X.df_input("maze", H, W) != 0).sum())
    assert n_valid == 2 * ((H + 1) // 2) * ((W + 1) // 2) - 1  # cells and the walls of a spanning tree
    all_go, all_stay = X.df_reference("maze", H, W, 0, n_valid, 1), X.df_reference("maze", H, W, 0, n_valid - 1, 1)
    a, b = all_go[3][0], all_stay[3][0]
    assert a.largest == n_valid and a.n_removed == n_valid and a.n_speckles == 1 and not all_go[0].any()
    assert b.largest == n_valid and b.n_removed == 0 and b.n_speckles == 0
    return n_valid, all_go, all_stay


@pytest.mark.parametrize("H,W", X.SIZES, ids=X.SIZE_IDS)
def test_filter_size_summed_over_every_tile(ctx, H, W):
    """the maze's size is the sum of the counts of its roots in all 256 tiles: one short or one over flips the removal"""
    n_valid, all_go, all_stay = summed_size_condition(H, W)
    img = X.df_input("maze", H, W)
    TD.check(TD.run(ctx, img, 0, n_valid, 1), all_go, f"maze {H}x{W} max_speckle_size n_valid")
    TD.check(TD.run(ctx, img, 0, n_valid - 1, 1), all_stay, f"maze {H}x{W} max_speckle_size n_valid - 1")


def levels_condition(name, median, d):
    H, W = X.SIZES[0]
    ref = X.df_reference(name, H, W, median, X.DF_LEVEL_SPECKLE, X.df_level_diff(name, d))
    info = ref[3][0]
    if (median, d) == (0, 0):    # no component is larger than the limit: everything goes
        assert info.largest <= X.DF_LEVEL_SPECKLE and info.n_removed == info.n_valid > 0 and info.n_components > 50000
    elif (median, d) == (5, 1):  # the median leaves the two middle levels: one component
        assert info.n_components == 1 and info.n_removed == 0
    else:
        assert 0 < info.n_removed < info.n_valid and 0 < info.n_speckles < info.n_components and info.n_components > 5000
    return ref


@pytest.mark.parametrize("median,d", X.DF_LEVEL_PARAMS, ids=[f"median {m} max_diff {d}" for m, d in X.DF_LEVEL_PARAMS])
@pytest.mark.parametrize("name", list(X.DF_OTHER))
def test_filter_many_components(ctx, name, median, d):
    H, W = X.SIZES[0]
    ref = levels_condition(name, median, d)
    diff = X.df_level_diff(name, d)
    TD.check(TD.run(ctx, X.df_input(name, H, W), median, X.DF_LEVEL_SPECKLE, diff), ref, f"{name} median {median} max_diff {diff}")


FRAMES = ("maze", "spiral", "serpentine", "maze")


def frames_case():
    H, W = X.SIZES[0]
    img = np.stack([X.df_input(n, H, W) for n in FRAMES])
    refs = [X.df_reference(n, H, W) for n in FRAMES]
    ref = tuple(np.stack([r[k] for r in refs]) for k in range(3)) + ([r[3][0] for r in refs],)
    assert all(i.n_components == 1 for i in ref[3]) and not np.array_equal(ref[0][0], ref[0][1])
    return img, ref


def test_filter_frames_stay_apart_under_load(ctx):
    import torch
    img, ref = frames_case()
    F, H, W = img.shape
    first = TD.run(ctx, img, 0, 100, 1, group_frames=0)
    TD.check(first, ref, "four frames, one group")
    for k in range(3):
        assert np.array_equal(first[k][0], first[k][3]), "frames 0 and 3 hold the same image"
    again = TD.run(ctx, img, 0, 100, 1, group_frames=0)
    assert all(first[k].tobytes() == again[k].tobytes() for k in range(3)) and first[3] == again[3], "a second call differs"
    TD.check(TD.run(ctx, img, 0, 100, 1, group_frames=3), ref, "four frames, groups of three")
    big = np.full((F, H + 3, W + 5), 0xEE, np.uint8)  # pitch and frame stride above the minimum
    pad = big[:, :H, :W]
    pad[...] = img
    assert pad.strides[0] > H * pad.strides[1] and pad.strides[1] > W and not pad.flags["C_CONTIGUOUS"]
    TD.check(TD.run(ctx, pad, 0, 100, 1), ref, "padded")
    TD.check(TD.run(ctx, pad, 0, 100, 1, group_frames=3), ref, "padded, groups of three")
    dev = TD.run(ctx, torch.from_numpy(img).cuda(), 0, 100, 1, group_frames=3)
    assert all(d.is_cuda for d in dev[:3])
    TD.check(dev, ref, "CUDA tensor")
    assert all(torch.equal(d[0], d[3]) for d in dev[:3])
    TD.check(TD.run(ctx, torch.from_numpy(big).cuda()[:, :H, :W], 0, 100, 1), ref, "CUDA tensor, padded")


SIDES = [(1, 8192), (8192, 1), (2, 8192), (8192, 2)]


@pytest.mark.parametrize("H,W", SIDES, ids=[f"{h}x{w}" for h, w in SIDES])
def test_filter_at_the_side_limit(ctx, H, W):
    """127 vertical tile borders of one or two pairs each (the row-by-row decoding of k_df_merge), or 511 horizontal ones;
    one row or one column of tiles"""
    img = X.df_input("levels uint8", H, W)
    ref = X.df_reference("levels uint8", H, W, 3, 3, 1)
    info = ref[3][0]
    assert 0 < info.n_removed < info.n_valid and info.n_components > 100
    TD.check(TD.run(ctx, img, 3, 3, 1), ref, f"{H}x{W}")


# ---- segmentation ------------------------------------------------------------------------------------------------------
def seg_run(ctx, case, **kw):
    name, H, W, step, m, K, min_size = case
    return TS.run(ctx, X.seg_input(name, H, W), step, m, K, min_size, **kw)


def random_condition(case):
    ref = X.seg_reference(*case)
    info = ref[3][0]
    assert 0 < info["n_merged"] < info["n_components"] and info["n_labels"] > 1000
    return ref


@pytest.mark.parametrize("case", X.SEG_RANDOM, ids=X.seg_id)
def test_segment_random_blocks(ctx, case):
    ref = random_condition(case)
    TS.check(seg_run(ctx, case), ref, X.seg_id(case))


def seg_winding_condition(case):
    """The largest component of equal raw labels lies in at least 100 tiles.  One case cannot meet that: a pixel's candidates
    are the centres of its home cell and the cells next to it, and after three updates of the 4 x 1 centres one colour's
    label changes at x = 512 and the other's at x = 768.  That cuts every turn of the spiral's arm, and of the dark arm
    between, in two: 257 components, the largest an arc of 1 783 pixels in 38 tiles.  (The maze's tree right of x = 512
    stays whole: 59 358 pixels in 127 tiles.)  An outer arc from x = 512 to the right edge, down the image and back
    covers 8 + 16 + 8 - 2 = 30 tiles at the least, which is what this case is held to, with more than 250 components."""
    ref = X.seg_reference(*case)
    pixels, tiles = X.tiles_of_largest_component(ref[1])
    what = f"{X.seg_id(case)}: the largest component has {pixels} pixels in {tiles} tiles"
    if case[0] == "spiral" and case[5] == 3:
        assert tiles >= 30 and ref[3][0]["n_components"] > 250, what
    else:
        assert tiles >= 100 and pixels > 10000, what
    return ref


@pytest.mark.parametrize("case", X.SEG_WINDING, ids=X.seg_id)
def test_segment_winding_components(ctx, case):
    """step 256, the contract's largest, never run otherwise: 4 x 1 centres whose seeds all lie on the bright colour.  With
    no update every distance ties and the labels are three rectangles; the updates pull the centres' colours apart, and
    the components follow the two colours through the tiles"""
    ref = seg_winding_condition(case)
    TS.check(seg_run(ctx, case), ref, X.seg_id(case))


def chain_condition():
    ref = X.seg_reference(*X.SEG_CHAIN)
    info = ref[3][0]
    assert info["n_components"] == 255 * 1023 and info["n_labels"] == 1 and info["n_merged"] == 255 * 1023 - 1
    assert info["largest"] == info["smallest"] == 255 * 1023 and not ref[0].any()
    return ref


def test_segment_longest_merge_chain(ctx):
    """checkerboard: every pixel is its own component, and all of them chain left and up to pixel 0: 260 864 adds on one
    count, link chains of up to W + H steps"""
    TS.check(seg_run(ctx, X.SEG_CHAIN), chain_condition(), X.seg_id(X.SEG_CHAIN))


def constant_condition():
    ref = X.seg_reference(*X.SEG_CONSTANT)
    info = ref[3][0]
    assert info["n_components"] == info["n_centres"] == info["n_labels"] == 32 * 128 and info["n_merged"] == 0
    return ref


def test_segment_constant_image_compact(ctx):
    TS.check(seg_run(ctx, X.SEG_CONSTANT), constant_condition(), X.seg_id(X.SEG_CONSTANT))


def large_y_condition():
    ref = X.seg_reference(*X.SEG_LARGE_Y)
    info = ref[3][0]
    assert info["n_centres"] == 2 * 1024 and 0 < info["n_merged"] < info["n_components"]
    return ref


def test_segment_large_y(ctx):
    """8192 x 9: y up to 8191 in the distances, the sums and the first pixels, 512 rows of tiles"""
    TS.check(seg_run(ctx, X.SEG_LARGE_Y), large_y_condition(), X.seg_id(X.SEG_LARGE_Y))


def seg_stack_case():
    img = np.stack([X.seg_input(c[0], c[1], c[2]) for c in X.SEG_STACK])
    refs = [X.seg_reference(*c) for c in X.SEG_STACK]
    ref = tuple(np.stack([r[k] for r in refs]) for k in range(3)) + ([r[3][0] for r in refs],)
    assert len({i["n_labels"] for i in ref[3]}) == 3  # three different frames
    return img, ref


def test_segment_stack_under_load(ctx):
    import torch
    img, ref = seg_stack_case()
    args = X.SEG_STACK[0][3:]
    first = TS.run(ctx, img, *args, group_frames=0)
    TS.check(first, ref, "three frames, one group")
    again = TS.run(ctx, img, *args, group_frames=0)
    assert all(first[k].tobytes() == again[k].tobytes() for k in range(3)) and first[3] == again[3], "a second call differs"
    TS.check(TS.run(ctx, img, *args, group_frames=2), ref, "three frames, groups of two")
    dev = TS.run(ctx, torch.from_numpy(img).cuda(), *args, group_frames=2)
    assert all(d.is_cuda for d in dev[:3])
    TS.check(dev, ref, "CUDA tensor")
