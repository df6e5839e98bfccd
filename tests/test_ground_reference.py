"""The numpy restatement of the ground filter's contract (ground_reference.py) does what a ground filter is for, on a scene
with a known answer: undulating ground, buildings and posts.  Runs without a GPU; the GPU tests then hold o3dr_ground_filter
to this reference bit for bit (test_ground_filter.py)."""
import numpy as np
import pytest

import ground_reference as gr
import raster_reference as rr

F32 = np.float32
SCHEDULES = {"exponential": dict(window_base=2, exponential=True), "linear": dict(window_base=4, exponential=False)}
_MEMO = {}


def scene_result(seed, sched, fill_radius):
    """computed once, shared, never written to"""
    key = (seed, sched, fill_radius)
    if key not in _MEMO:
        sc = _MEMO.setdefault(("scene", seed), gr.scene(seed))
        _MEMO[key] = gr.ground_filter(sc.xyz, gr.SCENE_CELL, bounds=gr.SCENE_BOX, fill_radius=fill_radius,
                                      **gr.SCENE_PARAMS, **SCHEDULES[sched])
    return _MEMO[("scene", seed)], _MEMO[key]


def test_schedule_values():
    r, t = gr.schedule(0.1, 32, 2, True, 0.3, 0.15, 2.0)
    assert r.tolist() == [1, 2, 4, 8, 16, 32] and r.dtype == np.int32 and t.dtype == F32
    want = [0.15] + [0.3 * (2 * d * 0.1) + 0.15 for d in (1, 2, 4, 8, 16)]
    assert np.array_equal(t, np.array(want, np.float64).astype(F32))
    r, t = gr.schedule(0.1, 32, 4, False, 0.3, 0.15, 2.0)
    assert r.tolist() == [4, 8, 12, 16, 20, 24, 28, 32] and np.array_equal(t[1:], np.full(7, 0.3 * (8 * 0.1) + 0.15).astype(F32))
    r, t = gr.schedule(0.5, 128, 2, True, 0.7, 0.15, 10.0)  # the cap: 0.7 * (2 * 64 * 0.5) + 0.15 > 10
    assert r.tolist() == [1, 2, 4, 8, 16, 32, 64, 128] and t[-1] == F32(10.0) and t[4] == F32(0.7 * (2 * 8 * 0.5) + 0.15)
    r, t = gr.schedule(0.05, 128, 1, False)  # at most 16 iterations
    assert r.tolist() == list(range(1, 17))
    r, t = gr.schedule(0.05, 1)
    assert r.tolist() == [1] and t.tolist() == [F32(0.15)]
    with pytest.raises(AssertionError):
        gr.schedule(0.05, 3, 4, False)


def test_window_is_the_plain_definition():
    rng = np.random.default_rng(5)
    a = rng.normal(0, 1, (9, 13)).astype(F32)
    for r in (1, 3, 20):
        got = gr.window(a, r, np.minimum, F32(np.inf))
        want = np.array([[a[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1].min() for x in range(13)] for y in range(9)])
        assert np.array_equal(got, want)
        assert np.array_equal(gr.window(a, r, np.maximum, F32(-np.inf)), -gr.window(-a, r, np.minimum, F32(np.inf)))


@pytest.mark.parametrize("sched", list(SCHEDULES))
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_scene_objects_go_and_ground_stays(seed, sched):
    sc, res = scene_result(seed, sched, 0)
    state, info = res.cell_state, res.info
    obj, gnd = sc.object & sc.present, ~sc.object & sc.present
    print(f"seed {seed} {sched}: object cells left {int((state[obj] == 1).sum())} of {int(obj.sum())}, "
          f"ground kept {100.0 * (state[gnd] == 1).mean():.3f} %, removed per iteration {info['n_removed']}")
    assert obj.sum() > 3000
    assert (state[obj] == 1).sum() == 0, "an object cell ends as ground"
    assert (state[gnd] == 1).mean() >= 0.999
    # the states, and the counts of step 8
    assert np.array_equal(state == 0, ~sc.present) and state.max() <= 1 + info["n_iterations"]
    assert info["n_removed"] == tuple(int((state == 2 + k).sum()) for k in range(info["n_iterations"]))
    assert info["n_occupied"] == int(sc.present.sum()) == info["n_ground_cells"] + sum(info["n_removed"])
    assert info["n_ground_cells"] + info["n_dtm_filled"] + info["n_dtm_empty"] == gr.SCENE_W * gr.SCENE_H
    assert info["n_inside"] == len(sc.xyz) and info["n_outside"] == 0 and info["n_dtm_filled"] == 0
    # one point per cell: the mask is the cells' outcome, and the DTM is Z on the ground cells, NaN elsewhere
    cx, cy = rr.cells_of(sc.xyz, gr.SCENE_CELL)
    cx, cy = cx - gr.SCENE_X0, cy - gr.SCENE_Y0
    assert np.array_equal(res.ground, (state[cy, cx] == 1).astype(np.uint8)) and info["n_ground_points"] == info["n_ground_cells"]
    assert np.array_equal(res.dtm[state == 1].view(np.uint32), res.Z[state == 1].view(np.uint32)) and np.isnan(res.dtm[state != 1]).all()
    assert np.array_equal(np.isnan(res.height_above_ground), state[cy, cx] != 1)
    assert (res.height_above_ground[res.ground == 1] == 0).all()


@pytest.mark.parametrize("sched", list(SCHEDULES))
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_scene_dtm_under_the_objects(seed, sched):
    """the ground's gradient is at most 0.036 + 0.15 m/m and the nearest ground cell under a 4 m building at most 2.1 m
    away: 0.39 m, plus the noise"""
    sc, res = scene_result(seed, sched, 32)
    plain = scene_result(seed, sched, 0)[1]
    assert np.array_equal(res.cell_state, plain.cell_state) and np.array_equal(res.ground, plain.ground)
    assert np.isfinite(res.dtm[sc.object]).all()
    err = np.abs(res.dtm[sc.object] - sc.truth[sc.object])
    print(f"seed {seed} {sched}: DTM error under the objects, max {err.max():.3f} m")
    assert err.max() <= 0.45
    on = res.cell_state == 1
    assert np.array_equal(res.dtm[on].view(np.uint32), res.Z[on].view(np.uint32))
    assert res.info["n_dtm_filled"] > 0 and res.info["n_ground_cells"] + res.info["n_dtm_filled"] + res.info["n_dtm_empty"] == on.size
    # heights above ground: an object's points stand 1 m (posts) or 2 - 4 m (roofs) above the DTM, give or take its error
    cx, cy = rr.cells_of(sc.xyz, gr.SCENE_CELL)
    h = res.height_above_ground[sc.object[cy - gr.SCENE_Y0, cx - gr.SCENE_X0]]
    assert np.isfinite(res.height_above_ground).all() and h.min() > 1.0 - 0.45 and h.max() < 4.0 + 0.45 + 0.6
