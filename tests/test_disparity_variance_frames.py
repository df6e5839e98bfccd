"""The variance gate (o3dr_disparity_variance, launch_disp_variance) past one launch of frames: the histogram kernel has the
frame in the grid's y extent, which holds 65 535, so the launcher issues one launch per 65 535 frames and moves `disp` and
`hist` by the first frame of each.  65 540 frames put five frames into a second launch."""
import numpy as np
import pytest

LAUNCH = 65535                     # frames per launch of k_disp_hist: a grid's y extent
BLOCK, N_BLOCKS = 5, 13108
N_FRAMES = BLOCK * N_BLOCKS        # 65 540
ROWS, COLS, BB = 4, 8, 1           # cs = cols / cutout_ratio = 1: the region of interest is rows 1 .. 2, columns 1 .. 6
MIN_DISPARITY = 64.0               # Params' default: a level takes part iff it is above


def base_block():
    """five frames of random levels around min_disparity; frame 3 lies entirely below it, frame 1 has it exactly"""
    rng = np.random.default_rng(65535)
    disp = rng.integers(40, 121, (BLOCK, ROWS, COLS)).astype(np.uint8)
    disp[3] = rng.integers(1, 65, (ROWS, COLS))
    disp[1, 1, 2] = 64
    disp[2, 2, 5] = 0
    return disp


def stacks():
    """the block tiled to 65 540 frames, and the same with the last block's frames in reverse order: the second launch then
    reads frames that differ from those at the start of the stack"""
    tiled = np.tile(base_block(), (N_BLOCKS, 1, 1))
    order = np.tile(np.arange(BLOCK), N_BLOCKS)
    order[-BLOCK:] = order[-BLOCK:][::-1]
    return tiled, np.ascontiguousarray(tiled[-BLOCK:][::-1]), order


def test_the_block_and_the_launch_boundary():
    disp = base_block()
    roi = disp[:, BB:ROWS - BB, COLS // 8:COLS - BB].astype(np.float64)
    assert roi.shape == (BLOCK, 2, 6)
    above = (roi > MIN_DISPARITY).reshape(BLOCK, -1).sum(axis=1)
    assert above[3] == 0 and (above[[0, 1, 2, 4]] > 0).all() and (above[[0, 1, 2, 4]] < 12).all()  # some at or below in every frame
    assert (roi == MIN_DISPARITY).any()
    assert N_FRAMES == 65540 and N_FRAMES - LAUNCH == 5 and LAUNCH % BLOCK == 0  # the second launch: the whole last block
    tiled, tail, order = stacks()
    assert tiled.shape == (N_FRAMES, ROWS, COLS) and order[LAUNCH:].tolist() == [4, 3, 2, 1, 0] and order[:BLOCK].tolist() == [0, 1, 2, 3, 4]
    assert not np.array_equal(tail, disp)


@pytest.mark.gpu
def test_variance_of_65540_frames(orc):
    import torch
    import online_3d_reconstruction_amd as o3dr
    disp = base_block()
    tiled, tail, order = stacks()
    with o3dr.Context(0, params=o3dr.Params(bounding_box=BB)) as c:
        base = c.disparityVariance(disp)
        ref = np.array([orc.disparity_variance(d, bounding_box=BB) for d in disp])
        rel = np.abs(base - ref) / np.maximum(ref, 1e-300)
        print(base, ref, rel)
        assert rel.max() <= 1e-9, rel  # (test_gpu_parity.py::test_disparity_variance_gate's tolerance)
        assert ref[3] == 0.0 and base[3] == 0.0 and (ref[[0, 1, 2, 4]] > 0).all() and len(set(base.tolist())) == BLOCK
        want = np.tile(base, N_BLOCKS)
        got = c.disparityVariance(tiled)
        assert got.shape == (N_FRAMES,) and np.array_equal(got.view(np.uint64), want.view(np.uint64)), "host"
        got = c.disparityVariance(torch.from_numpy(tiled).cuda())
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), "device"
        tiled[-BLOCK:] = tail
        want = base[order]
        got = c.disparityVariance(tiled)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), "host, last block reversed"
        got = c.disparityVariance(torch.from_numpy(tiled).cuda())
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), "device, last block reversed"
