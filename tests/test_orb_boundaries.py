"""ORB detection (o3dr_orb_detect; Context.findFeatures) past the sizes of tests/test_orb_features.py: a second round of
the chunk scan and of the selection's compaction, ties of the cut value spread over several rounds, a cut among negative
Harris responses, quota 0 on a level with candidates, levels that do not exist, the FAST arc at 8 / 9 pixels and at a
contrast of thr / thr + 1, sources that start off a word boundary, several frame groups, more than 256 (frame, level)
segments.

Every comparison is exact against tests/orb_reference.py (integers and IEEE-exact floats).  Every GPU test has a CPU
twin (or in-test assertions) that shows with the restatement alone that its input reaches the boundary it is named for:
those say nothing about the library."""
import ctypes as C

import numpy as np
import pytest

import orb_reference as ref
from conftest import load_frame

CHUNK = 1024   # pixels per chunk of the candidate passes (kOrbChunk)
ROUND = 256    # chunks per round of k_orb_scan, candidates per round of k_orb_select, segments per round of k_orb_offsets


def _lib():
    from online_3d_reconstruction_amd import _lib as L
    return L, L.load_library()


def _grey():
    return ref.grey(load_frame("1248")[1])


def _big():
    """600 x 520 = 312 000 pixels: 305 chunks, so the scan of level 0 takes two rounds"""
    return np.ascontiguousarray(_grey()[60:660, 380:900])


def _negatives():
    """a 160 x 160 window of _big() that is rich in negative Harris responses at fast_threshold = 5, edge = 16"""
    return np.ascontiguousarray(_big()[100:260, 200:360])


def _crop(y=300, x=600, n=192):
    return np.ascontiguousarray(load_frame("1248")[1][y:y + n, x:x + n])


_MEMO = {}


def _memo(key, make):
    """a reference value, computed once and shared; nobody writes to it"""
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def _detect(name, make, **kw):
    return _memo((name,) + tuple(sorted(kw.items())), lambda: ref.detect(make(), **kw))


def _stage(name, make, thr, edge):
    """-> (ys, xs, R) of level 0's candidates in row-major order"""
    def run():
        g = make()
        ys, xs = ref.candidates(ref.fast_scores(g, thr), edge)
        return ys, xs, ref.harris(g, ys, xs)
    return _memo(("stage", name, thr, edge), run)


def _bytes(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _assert_equal(got, want, what):
    kp, xy, desc = got[:3]
    assert len(kp) == len(want["kp"]), f"{what}: {len(kp)} keypoints, reference {len(want['kp'])}"
    for name in ref.KEYPOINT.names:
        a, b = np.ascontiguousarray(kp[name]), np.ascontiguousarray(want["kp"][name])
        bad = np.nonzero(a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1))[0]
        assert bad.size == 0, f"{what}: field {name} differs at {bad[:5]}: {a[bad[:5]]} vs {b[bad[:5]]}"
    assert np.array_equal(np.asarray(xy).view(np.uint32), want["kp_xy"].view(np.uint32)), f"{what}: kp_xy"
    assert np.array_equal(desc, want["desc"]), f"{what}: descriptors differ in rows {np.nonzero((desc != want['desc']).any(1))[0][:5]}"


def _assert_levels(got_levels, want, what):
    flat = np.concatenate([lv.reshape(-1) for lv in want["levels"]])
    assert len(got_levels) == len(flat), f"{what}: {len(got_levels)} pyramid bytes, reference {len(flat)}"
    bad = np.nonzero(np.asarray(got_levels) != flat)[0]
    assert bad.size == 0, f"{what}: pyramid differs at byte {bad[0]} of {[lv.size for lv in want['levels']]}"


def _assert_same(a, b, what):
    """two findFeatures results (any memory kind), byte for byte"""
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(_bytes(x), _bytes(y)), f"{what}: output {k} differs"


# ---- 1. a second scan round and a second select round --------------------------------------------------------------------
SCAN_CASES = {"cut300": dict(n_features=300, n_levels=1), "all5000": dict(n_features=5000, n_levels=1),
              "levels3": dict(n_features=600, n_levels=3)}


def test_the_big_crop_needs_two_scan_rounds_and_ten_select_rounds():
    g = _big()
    assert g.shape == (600, 520) and -(-g.size // CHUNK) == 305 > ROUND
    ys, xs, _ = _stage("big", _big, 20, 31)
    chunk = (ys * g.shape[1] + xs) // CHUNK
    assert len(ys) == 2498 and int((chunk >= ROUND).sum()) == 279
    assert len(ys) > 9 * ROUND  # the compaction of level 0 takes ten rounds
    wh, quota = ref.level_sizes(600, 520, 600, 1.3, 3)
    assert quota[0] < 2498 and all(-(-w * h // CHUNK) <= ROUND for w, h in wh[1:])


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(SCAN_CASES))
def test_second_scan_round_and_select_rounds(ctx, case):
    kw = SCAN_CASES[case]
    want = _detect("big", _big, **kw)
    assert want["n_candidates"][0] == 2498
    if case == "cut300":
        assert len(want["kp"]) == 300
        slot = (want["kp"]["yl"].astype(np.int64) * 520 + want["kp"]["xl"]) // CHUNK
        assert (slot >= ROUND).any() and (slot < ROUND).any()  # kept candidates on both sides of the scan's round
    elif case == "all5000":
        assert len(want["kp"]) == 2498  # n <= quota: no selection
    else:
        lv = want["kp"]["level"]
        assert len(want["levels"]) == 3 and (lv == 0).sum() < 2498 and (lv == 1).any() and (lv == 2).any()
    got = ctx.findFeatures(_big(), return_levels=True, **kw)
    _assert_levels(got[4], want, case)
    _assert_equal(got, want, case)
    assert got[3].tolist() == [0, len(want["kp"])]


# ---- 2. low threshold, the smallest margin, negative responses -----------------------------------------------------------
LOW = dict(fast_threshold=5, edge=16, n_levels=1)


def _cut_among_negatives():
    _, _, R = _stage("neg", _negatives, 5, 16)
    return int((R >= 0).sum() + (R < 0).sum() // 2)


def test_the_low_threshold_inputs_have_negative_responses_on_both_sides_of_the_cut():
    _, _, R = _stage("biglow", _big, 5, 16)
    assert len(R) == 11031 and int((R < 0).sum()) == 163
    _, _, R = _stage("neg", _negatives, 5, 16)
    n = _cut_among_negatives()
    assert ROUND < n < len(R)  # the cut is still found over more than one round of candidates
    want = _detect("neg", _negatives, n_features=n, **LOW)
    kept = int((want["kp"]["response"] < 0).sum())
    assert len(want["kp"]) == n and kept >= 8 and int((R < 0).sum()) - kept >= 8
    assert int((R == 0).sum()) == 0 and int((want["kp"]["response"] > 0).sum()) == int((R > 0).sum())


@pytest.mark.gpu
def test_low_threshold_small_margin(ctx):
    want = _detect("biglow", _big, n_features=400, **LOW)
    assert want["n_candidates"] == [11031] and len(want["kp"]) == 400
    assert want["kp"]["xl"].min() < 31 or want["kp"]["yl"].min() < 31  # inside the default margin: edge = 16 matters
    _assert_equal(ctx.findFeatures(_big(), n_features=400, **LOW), want, "threshold 5, edge 16")


@pytest.mark.gpu
def test_cut_among_negative_responses(ctx):
    n = _cut_among_negatives()
    want = _detect("neg", _negatives, n_features=n, **LOW)
    kept = int((want["kp"]["response"] < 0).sum())
    assert kept >= 8 and len(want["kp"]) == n < want["n_candidates"][0]
    _assert_equal(ctx.findFeatures(_negatives(), n_features=n, **LOW), want, "cut among negatives")


# ---- 3. ties of the cut value across select rounds ------------------------------------------------------------------------
def _dots():
    rng = np.random.default_rng(1)
    img = np.full((256, 256), 30, np.uint8)
    for y in range(20, 236, 8):
        for x in range(20, 236, 8):
            img[y, x] = rng.choice([120, 200])
    return img


TIE_CUTS = [100, 357, 358, 357 + 186, 728]


def test_the_dots_tie_in_two_groups_that_span_every_round():
    _, _, R = _stage("dots", _dots, 20, 16)
    vals, counts = np.unique(R, return_counts=True)
    assert len(R) == 729 and counts.tolist() == [372, 357] and vals[0] > 0
    for v in vals:  # whichever value the cut falls on, its ties lie in round 0 and in round 2
        idx = np.nonzero(R == v)[0]
        assert idx.min() < ROUND and idx.max() > 2 * ROUND
    # 357 + 186: the kept low ties end inside a round, the cut's ties begin before round 1
    low = np.nonzero(R == vals[0])[0]
    assert low[0] < ROUND and low[185] % ROUND not in (0, ROUND - 1) and low[185] > ROUND


@pytest.mark.gpu
@pytest.mark.parametrize("n", TIE_CUTS)
def test_ties_across_select_rounds(ctx, n):
    want = _detect("dots", _dots, n_features=n, n_levels=1, edge=16)
    assert want["n_candidates"] == [729] and len(want["kp"]) == n
    got = ctx.findFeatures(_dots(), n_features=n, n_levels=1, edge=16)
    _assert_equal(got, want, f"dots, quota {n}")
    assert got[3].tolist() == [0, n]


# ---- 4. quota 0 on a level with candidates; levels that do not exist; level sizes ------------------------------------------
def _strip():
    return np.ascontiguousarray(_grey()[300:363, 600:800])  # 63 x 200


STRIP = dict(n_features=200, scale_factor=2.0, n_levels=8, edge=16)


def test_quota_zero_and_missing_level_inputs():
    wh, quota = ref.level_sizes(192, 192, 1, 1.3, 3)
    assert quota == [1, 0, 0]
    want = _detect("crop", _crop, n_features=1, n_levels=3)
    assert want["n_candidates"][1] > 0 and want["n_candidates"][2] > 0 and len(want["kp"]) == 1
    wh, quota = ref.level_sizes(63, 200, 200, 2.0, 8)
    assert wh[6] == (3, 1) and wh[7] == (0, 0) and quota[7] == 0
    want = _detect("strip", _strip, **STRIP)
    assert len(want["levels"]) == 7 and want["n_candidates"][0] > 0 and len(want["kp"]) > 0


@pytest.mark.gpu
def test_quota_zero_on_a_level_with_candidates(ctx):
    want = _detect("crop", _crop, n_features=1, n_levels=3)
    assert want["n_candidates"][1] > 0
    got = ctx.findFeatures(_crop(), n_features=1, n_levels=3, return_levels=True)
    _assert_equal(got, want, "quotas 1, 0, 0")
    assert len(got[0]) == 1 and got[3].tolist() == [0, 1]
    _assert_levels(got[4], want, "quotas 1, 0, 0")


@pytest.mark.gpu
def test_levels_that_do_not_exist(ctx):
    want = _detect("strip", _strip, **STRIP)
    got = ctx.findFeatures(_strip(), return_levels=True, **STRIP)
    _assert_levels(got[4], want, "63 x 200, 8 levels of factor 2")
    _assert_equal(got, want, "63 x 200, 8 levels of factor 2")
    assert got[3].tolist() == [0, len(want["kp"])]


def test_level_sizes_at_the_corners_of_the_parameters():
    L, lib = _lib()
    for rows, cols in ((63, 200), (720, 1280), (8192, 8192), (1, 1)):
        for sf in (1.01, 1.2, 1.3, 2.0):
            for nl in (1, 5, 8):
                for nf in (1, 1500, 65535):
                    prm = L.OrbParamsStruct(nf, sf, nl, 20, 31, 1)
                    wh, quota = np.full(2 * nl, -1, np.int32), np.full(nl, -1, np.int32)
                    assert lib.o3dr_orb_level_sizes(rows, cols, C.byref(prm), wh.ctypes.data, quota.ctypes.data) == 0
                    rwh, rq = ref.level_sizes(rows, cols, nf, sf, nl)
                    what = (rows, cols, sf, nl, nf)
                    assert wh.reshape(nl, 2).tolist() == [list(x) for x in rwh], what
                    assert quota.tolist() == rq and int(quota.sum()) == nf and (quota >= 0).all(), what
                    assert wh[0] == cols and wh[1] == rows, what
                    for l in range(nl):
                        w, h = int(wh[2 * l]), int(wh[2 * l + 1])
                        assert (w > 0) == (h > 0), what
                        if w == 0:  # a missing level: (0, 0), nothing to find, and every later level is missing too
                            assert quota[l] == 0 and not wh[2 * l:].any(), what
    # (cases above do have missing levels: half a pixel still rounds up to one)
    assert ref.level_sizes(1, 1, 1, 2.0, 8)[0] == [(1, 1), (1, 1)] + [(0, 0)] * 6


# ---- 5. FAST arcs ------------------------------------------------------------------------------------------------------
PITCH, FIRST, PER_ROW = 24, 28, 12


def _stamps():
    """(arc length, first ring index, polarity, contrast): bright ones first, then dark ones, a row of the grid never mixes"""
    out = []
    for pol in (1, -1):
        out += [(n, s, pol, c) for c in (20, 21) for n in (8, 9) for s in range(16)]
        if pol == 1:
            out += [(9, 3, 1, 155), (9, 14, 1, 200)]  # 100 + 155 = 255 exactly, and 100 + 200 clipped to 255
            out += [None] * (-len(out) % PER_ROW)
    return out


def _centre(k):
    return FIRST + PITCH * (k // PER_ROW), FIRST + PITCH * (k % PER_ROW)


def _arcs(binary):
    """binary = False: background 100, arcs at 100 +- c.  binary = True: the bright stamps' rows are 0 with arcs of 255, the
    dark stamps' rows 255 with arcs of 0 - every contrast is 255"""
    st = _stamps()
    rows = -(-len(st) // PER_ROW)
    img = np.full((2 * FIRST + PITCH * (rows - 1), 2 * FIRST + PITCH * (PER_ROW - 1)), 100, np.int64)
    if binary:
        first_dark = next(k for k, s in enumerate(st) if s is not None and s[2] < 0)
        split = _centre(first_dark)[0] - PITCH // 2
        img[:split], img[split:] = 0, 255
    for k, s in enumerate(st):
        if s is None:
            continue
        n, start, pol, c = s
        y, x = _centre(k)
        for i in range(n):
            dx, dy = ref.RING[(start + i) % 16]
            img[y + dy, x + dx] = (255 if pol > 0 else 0) if binary else min(255, 100 + pol * c)
    return img.astype(np.uint8)


ARC_CASES = {"grey": (False, 20), "binary": (True, 254)}
ARC_KW = dict(n_features=4000, n_levels=1, edge=16)


def test_the_arc_stamps_pass_and_fail_where_they_should():
    st = _stamps()
    real = [s for s in st if s is not None]
    for pol in (1, -1):
        for c in (20, 21):
            got = {(n, s) for n, s, p, cc in real if p == pol and cc == c}
            assert got == {(n, s) for n in (8, 9) for s in range(16)}  # 8 and 9 at every start, the wrap 15 -> 0 among them
    assert PITCH - 7 > 2 * 3 + 2  # isolated: no ring (radius 3) reaches two stamps (7 wide), scores of two stamps never touch
    grey = _arcs(False)
    assert grey.max() == 255 and grey.min() == 79 and grey.shape[0] * grey.shape[1] < ROUND * CHUNK
    s = ref.fast_scores(grey, 20)
    for k, stamp in enumerate(st):
        if stamp is None:
            continue
        n, start, pol, c = stamp
        y, x = _centre(k)
        assert min(y, x) >= 16 and y < grey.shape[0] - 16 and x < grey.shape[1] - 16
        if n == 9 and c >= 21:
            assert s[y, x] == min(c, 155), stamp  # 21, or the saturated 255 - 100
        else:
            assert s[y, x] == 0, stamp  # an arc of 8, or a contrast of exactly the threshold
    b = _arcs(True)
    assert set(np.unique(b)) == {0, 255}
    s = ref.fast_scores(b, 254)
    assert set(np.unique(s)) == {0, 255}
    for k, stamp in enumerate(st):
        if stamp is not None:
            y, x = _centre(k)
            assert s[y, x] == (255 if stamp[0] == 9 else 0), stamp
    for name, (binary, thr) in ARC_CASES.items():
        want = _detect("arcs" + name, lambda: _arcs(binary), fast_threshold=thr, **ARC_KW)
        assert 0 < want["n_candidates"][0] == len(want["kp"]) < ARC_KW["n_features"]  # nothing is cut: every corner is compared


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(ARC_CASES))
def test_fast_arcs(ctx, case):
    binary, thr = ARC_CASES[case]
    want = _detect("arcs" + case, lambda: _arcs(binary), fast_threshold=thr, **ARC_KW)
    got = ctx.findFeatures(_arcs(binary), fast_threshold=thr, **ARC_KW)
    _assert_equal(got, want, f"arc stamps, {case}")


# ---- 6. sources that start off a word boundary ------------------------------------------------------------------------------
UNALIGNED_KW = dict(n_features=200, n_levels=2, return_levels=True)


def _unaligned(ch, batch):
    """-> (view, contiguous copy): 200 x 260 pixels that start one column into 200 x 261 (3 frames: 203 x 261 each)"""
    src = load_frame("1248")[1] if ch == 3 else _grey()
    wide = [np.ascontiguousarray(src[250 + 40 * f:453 + 40 * f, 500 + 30 * f:761 + 30 * f]) for f in range(3)]
    if batch:
        big = np.stack(wide)
        view = big[:, :200, 1:]
    else:
        big = wide[0][:200]
        view = big[:, 1:]
    return big, view


def test_the_unaligned_views_are_unaligned():
    for ch in (1, 3):
        for batch in (False, True):
            big, view = _unaligned(ch, batch)
            assert view.ctypes.data - big.ctypes.data == ch and view.strides[-1 - (ch == 3)] == ch
            assert view.strides[-2 - (ch == 3)] == 261 * ch and view.shape[-2 - (ch == 3):][:2] == (200, 260)
            assert not view.flags.c_contiguous
            if batch:
                assert view.strides[0] == 203 * 261 * ch > 200 * 261 * ch and view.shape[0] == 3
    g = _unaligned(1, False)[1]
    assert np.array_equal(ref.grey(_unaligned(3, False)[1]), g)


@pytest.mark.gpu
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("batch", [False, True], ids=["one", "batch"])
def test_unaligned_sources(ctx, ch, batch):
    import torch
    big, view = _unaligned(ch, batch)
    copy = np.ascontiguousarray(view)
    want = ctx.findFeatures(copy, **UNALIGNED_KW)
    n0 = 200 * 260
    frames = copy if batch else copy[None]
    assert len(want[0]) > 0 and (np.diff(want[3]) > 0).all()
    per_frame = len(want[4]) // len(frames)
    for f, fr in enumerate(frames):  # level 0 is the grey image itself
        assert np.array_equal(want[4][f * per_frame:f * per_frame + n0], (ref.grey(fr) if ch == 3 else fr).reshape(-1))
    _assert_same(ctx.findFeatures(view, **UNALIGNED_KW), want, "host view")
    dbig = torch.from_numpy(big).cuda()
    dview = dbig[:, :200, 1:] if batch else dbig[:, 1:]
    assert dview.data_ptr() - dbig.data_ptr() == ch and not dview.is_contiguous()
    _assert_same(ctx.findFeatures(dview, **UNALIGNED_KW), want, "device view")
    _assert_same(ctx.findFeatures(torch.from_numpy(copy).cuda(), **UNALIGNED_KW), want, "device copy")


# ---- 7. frame groups ---------------------------------------------------------------------------------------------------------
GROUP_KW = dict(n_features=64, n_levels=2, return_levels=True)


def _group_frames():
    flat = np.full((192, 192, 3), 90, np.uint8)
    return np.stack([_crop(300, 600), _crop(200, 500), flat, _crop(304, 607), _crop(300, 600)])


def test_the_scratch_limit_hook_needs_a_context():
    _, lib = _lib()
    assert lib.o3dr_test_orb_scratch_limit(None, 0) == -1


@pytest.mark.gpu
def test_frame_groups(monkeypatch):
    import torch

    import online_3d_reconstruction_amd as o3dr
    L, lib = _lib()
    frames = _group_frames()
    monkeypatch.delenv("O3DR_TEST_HOOKS", raising=False)
    with o3dr.Context(0) as c:
        assert lib.o3dr_test_orb_scratch_limit(c._h, 1 << 20) == L.ERR_INVALID_ARG
        assert b"test hooks are off" in lib.o3dr_last_error()
    monkeypatch.setenv("O3DR_TEST_HOOKS", "1")
    with o3dr.Context(0) as c:
        c.profileEnable(L.K_ORB_SELECT)

        def run(img, limit):
            """-> (result, groups): one selection pass is bracketed per group"""
            L.check(lib.o3dr_test_orb_scratch_limit(c._h, limit))
            c.profileReset()
            out = c.findFeatures(img, **GROUP_KW)
            return out, c.profileRead(L.K_ORB_SELECT)[1]

        assert lib.o3dr_test_orb_scratch_limit(c._h, -1) == L.ERR_INVALID_ARG
        singles = [run(f, 0)[0] for f in frames]
        counts = [len(s[0]) for s in singles]
        assert counts[2] == 0 and min(counts[0], counts[1], counts[3]) > 0 and counts[4] == counts[0]
        _assert_equal(singles[0], _detect("crop2", _crop, n_features=64, n_levels=2), "first frame")
        joined = [np.concatenate([_bytes(s[k]) for s in singles]) for k in (0, 1, 2, 4)]
        dframes = torch.from_numpy(frames).cuda()
        # (two frames of this size need 625 168 bytes of scratch, three 937 752)
        for limit, groups in ((0, 1), (700_000, 3), (1, 5), (0, 1)):
            for img in (frames, dframes):
                got, n_groups = run(img, limit)
                what = f"limit {limit}, {'device' if img is dframes else 'host'}"
                assert n_groups == groups, f"{what}: {n_groups} groups"
                assert got[3].tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist(), what
                for k, want in zip((0, 1, 2, 4), joined):
                    assert np.array_equal(_bytes(got[k]), want), f"{what}: output {k} differs from the per-frame calls"


# ---- 8. more than 256 (frame, level) segments ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("edge", [31, 16])
def test_more_than_256_segments(ctx, edge):
    g = _grey()
    crops = [np.ascontiguousarray(g[y:y + 128, x:x + 160]) for y, x in ((300, 600), (200, 500), (340, 700), (260, 420))]
    flat = np.full((128, 160), 77, np.uint8)
    which = [4 if f % 5 == 4 else (f - f // 5) % 4 for f in range(40)]
    assert which[:10] == [0, 1, 2, 3, 4, 0, 1, 2, 3, 4] and which[10:15] == [0, 1, 2, 3, 4]
    frames = np.stack([(crops + [flat])[w] for w in which])
    kw = dict(n_features=40, scale_factor=1.2, n_levels=8, edge=edge, return_levels=True)
    assert len(frames) * kw["n_levels"] == 320 > ROUND
    singles = [ctx.findFeatures(im, **kw) for im in crops + [flat]]
    counts = [len(s[0]) for s in singles]
    assert min(counts[:4]) > 0 and counts[4] == 0
    want = _detect("seg0", lambda: crops[0], n_features=40, scale_factor=1.2, n_levels=8, edge=edge)
    _assert_equal(singles[0], want, "first crop alone")
    _assert_levels(singles[0][4], want, "first crop alone")
    if edge == 16:
        assert len(set(want["kp"]["level"].tolist())) >= 4  # many live segments per frame
    got = ctx.findFeatures(frames, **kw)
    off = np.concatenate([[0], np.cumsum([counts[w] for w in which])])
    assert got[3].tolist() == off.tolist()
    per_frame = len(singles[0][4])
    for f, w in enumerate(which):
        for k in (0, 1, 2):
            assert np.array_equal(_bytes(got[k][off[f]:off[f + 1]]), _bytes(singles[w][k])), f"frame {f}: output {k}"
        assert np.array_equal(got[4][f * per_frame:(f + 1) * per_frame], singles[w][4]), f"frame {f}: pyramid"
