"""tests/multiview_fuse_reference.py checked alone, on the CPU: the fused levels are nearer the real-valued ones than the
quantised input is, and the three identities that tie the fusion to the filter (include/o3dr.h "multi-view fusion") hold
on the filter tests' multi-tile scenes."""
import numpy as np
import pytest

import multiview_fuse_reference as RF
import multiview_reference as R
from test_multiview_filter import MULTI_TILE, scene

_ids = ["%dx%d-F%d-k%d-%s-t%g-s%d-v%d" % (c[:4] + (np.dtype(c[4]).name,) + c[5:8]) for c in MULTI_TILE]


def test_fused_levels_are_nearer_the_real_ones_than_the_quantised_input():
    disp, Q, poses, real = R.plane_scene(48, 64, 5, 1, np.uint8, max_shift=0.08)
    nb = R.nearby_frames(poses, 4)
    out, votes, _, _, infos = RF.multiview_fuse(disp, Q, poses, nb)
    kept = out > 0
    lv, valid = R.levels(disp)
    rms_in = float(np.sqrt(np.mean((lv[kept] - real[kept]) ** 2)))
    rms_out = float(np.sqrt(np.mean((out[kept] - real[kept]) ** 2)))
    print("rms: input %.4f, fused %.4f, ratio %.3f; kept %.3f of the valid pixels, %.2f votes per kept pixel"
          % (rms_in, rms_out, rms_out / rms_in, kept.sum() / valid.sum(), votes[kept].mean()))
    assert kept.sum() > 0.5 * valid.sum()
    assert rms_out < 0.75 * rms_in
    assert sum(i.n_fused for i in infos) > 0


@pytest.mark.parametrize("c", MULTI_TILE, ids=_ids)
def test_the_three_identities_and_the_vote_counts(c):
    rows, cols, F, k, dtype, tol, ms, mv_, seed = c
    disp, Q, poses = scene(rows, cols, F, seed, dtype)
    nb = R.nearby_frames(poses, k)
    f_out, f_sup, f_vio, f_info = R.multiview_filter(disp, Q, poses, nb, tol, ms, mv_)
    out, votes, sup, vio, infos = RF.multiview_fuse(disp, Q, poses, nb, tol, ms, mv_)
    assert out.dtype == np.float64 and votes.dtype == np.uint8
    assert np.array_equal(out > 0, f_out != 0)
    assert np.isfinite(out).all() and (out >= 0).all()
    assert np.array_equal(sup, f_sup) and np.array_equal(vio, f_vio) and [i.filter for i in infos] == f_info
    assert (votes <= sup).all()
    for f, i in enumerate(infos):
        assert i.n_votes + i.n_votes_dropped == i.filter.n_support
        assert i.n_votes == int(votes[f].astype(np.int64).sum())
        assert i.n_fused == int(((out[f] > 0) & (votes[f] > 0)).sum())
    # tolerance = 0: no test is a support, so the fusion is the filtered image's levels exactly
    z_out = RF.multiview_fuse(disp, Q, poses, nb, 0.0, ms, mv_)[0]
    z_lv, z_valid = R.levels(R.multiview_filter(disp, Q, poses, nb, 0.0, ms, mv_)[0])
    assert np.array_equal(z_out.view(np.uint8), np.where(z_valid, z_lv, 0.0).view(np.uint8))
    # a kept pixel without a vote returns its own level exactly
    lv, _ = R.levels(disp)
    lone = (out > 0) & (votes == 0)
    assert np.array_equal(out[lone], lv[lone])
