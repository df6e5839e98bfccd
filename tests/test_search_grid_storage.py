"""The search grid owns its storage (DESIGN.md "Scratch contract": `ws_grid_block` next to `ws_sor_block`).

The grid that nearest neighbours, ICP, MLS and the clustering search is carved on its own; the arrays of the statistical
outlier removal (inliers, distances, handed-over queries: 24 bytes a point) exist only once an outlier removal has run.
The two blocks grow independently, so a grid that grows between two outlier removals - and an outlier removal between two
searches - must leave every result as it was."""
import numpy as np
import pytest

from conftest import assert_points_equal
from test_icp_align import _pts, _torch_pts
from test_scratch_independence import fill, hooked_context
from test_search_grid_stress import map_like

N_SOR = 20000    # above kSmallMax = 8192: launch_sor; above 2048: max_cells = n / 2
N_GROW = 4100    # max_cells 2050: past the 1024 cells of a grid carved for at most 2048 points


def _cloud(n):
    nx = {N_SOR: 200, N_GROW: 82}[n]
    xyz = map_like(nx, n // nx, seed=n)
    assert len(xyz) == n
    return _pts(xyz)


def _nn_bits(r):
    return np.asarray(r[0]).view(np.uint32).tobytes(), np.asarray(r[1]).view(np.uint32).tobytes()


@pytest.mark.gpu
def test_a_map_operator_allocates_no_outlier_removal_arrays():
    """nearest neighbours of 20 000 device points, then the outlier removal of the same points: the scratch the context owns
    grows by the removal's own per-point arrays (sor_pts 16 + sor_dist 4 + sor_left 4 bytes a point) only then"""
    cloud = _torch_pts(_cloud(N_SOR))
    with hooked_context() as ctx:
        idx, _ = ctx.nearestNeighbors(cloud, cloud)
        assert np.array_equal(idx.cpu().numpy().view(np.uint32), np.arange(N_SOR, dtype=np.uint32))
        b1 = fill(ctx, 0)
        kept = ctx.statisticalOutlierRemoval(cloud)
        assert 0 < len(kept) <= N_SOR
        b2 = fill(ctx, 0)
    print(f"scratch after nearestNeighbors {b1} bytes, after statisticalOutlierRemoval {b2} bytes, n = {N_SOR}")
    assert b2 - b1 >= 24 * N_SOR, (b1, b2)


@pytest.mark.gpu
def test_the_grid_may_grow_between_two_batched_outlier_removals():
    """two frames through the batched outlier removal on grids of 1024 cells (stride 1025 between the frames); a
    4100-point nearest-neighbour target then re-carves the grids' block for 2050 cells; the same two frames again give the
    same merged cloud byte for byte"""
    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import synth
    rows, cols = 96, 128
    disp, bgr = synth.make_frames(0, 2, rows, cols)
    poses = synth.make_poses(0, 2)
    target = _cloud(N_GROW)
    with hooked_context() as ctx:
        ctx.set_camera(synth.camera_Q(rows, cols))
        ctx.set_params(o3dr.Params(jump_pixels=2, sor_enable=True))
        assert 50 < ctx.max_points(rows, cols) <= 2048  # more than mean_k points; the grid's floor of 1024 cells

        def merged():
            ctx.cloudBigReset()
            ctx.accumulateFrames(disp, bgr, poses)
            return ctx.finalize()

        first = merged()
        assert len(first) > 0
        ctx.nearestNeighbors(target, target)
        assert_points_equal(merged(), first, "merged cloud after the grid grew")


@pytest.mark.gpu
def test_an_outlier_removal_between_two_searches_of_a_smaller_grid():
    """the mirror image: nearest neighbours in 4100 points, the outlier removal of 20 000 points (both blocks grow), the
    same search again: idx and d2 byte for byte"""
    small, big = _cloud(N_GROW), _cloud(N_SOR)
    with hooked_context() as ctx:
        first = _nn_bits(ctx.nearestNeighbors(small, small))
        assert 0 < len(ctx.statisticalOutlierRemoval(big)) <= N_SOR
        assert _nn_bits(ctx.nearestNeighbors(small, small)) == first
    assert np.array_equal(np.frombuffer(first[0], np.uint32), np.arange(N_GROW, dtype=np.uint32))
