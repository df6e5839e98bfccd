"""CPU tests of the contour-line contract itself (include/o3dr_contour.h) on its numpy restatement,
tests/contour_reference.py: known answers of a prototype of the contract, and the invariants every result must keep."""
import numpy as np
import pytest

import contour_reference as cr


def noise():
    rng = np.random.default_rng(1)
    Z = (rng.normal(size=(40, 50)) * 2).astype(np.float32)
    Z[rng.random(Z.shape) < 0.05] = np.nan
    return rng, Z


def cone(n=64, cx=31.3, cy=30.8, radius=30.0):
    y, x = np.mgrid[0:n, 0:n]
    return (radius - np.hypot(x - cx, y - cy)).astype(np.float32)


def plane():
    y, x = np.mgrid[0:20, 0:24]
    return (0.25 * x + 0.5 * y + 3).astype(np.float32)


def integers():
    rng, _ = noise()
    return rng.integers(0, 4, (12, 12)).astype(np.float32)


MULTI = np.array([[0, 10], [0.3, 7]], np.float32)

# The 18 case resolutions of one quad as 2 x 2 rasters [[b0, b1], [b3, b2]] at the level 0.5 (k = 0 of base 0.5, interval 1):
# bit i of `bits` = corner b_i inside.  An inside corner is 0.75, an outside one 0; the saddles (5: b0, b2 inside; 10: b1, b3)
# then have the centre 0.375, outside, and with the inside pair at 3 the centre 1.5, inside.
CASES = []
for bits in range(16):
    for high, centre_in in ((0.75, False), (3.0, True)) if bits in (5, 10) else ((0.75, None),):
        b = [high * ((bits >> i) & 1) for i in range(4)]
        CASES.append((bits, centre_in, np.array([[b[0], b[1]], [b[3], b[2]]], np.float32)))
assert len(CASES) == 18


def check_invariants(Z, seg, lines, vertices, info):
    S, H, W = len(seg), Z.shape[0], Z.shape[1]
    assert info["n_segments"] == S and info["n_lines"] == len(lines) and info["n_vertices"] == S + len(lines) == len(vertices)
    if S == 0:
        return
    nxt = seg["next"].astype(np.int64)
    linked = np.nonzero(nxt >= 0)[0]
    for a, b in (("x1", "x0"), ("y1", "y0")):  # i's end is next[i]'s start, bitwise
        assert np.array_equal(seg[a][linked].view(np.uint64), seg[b][nxt[linked]].view(np.uint64))
    assert len(np.unique(nxt[linked])) == len(linked)  # prev is a function
    assert np.array_equal(seg["k"][linked], seg["k"][nxt[linked]])
    assert np.array_equal(lines["k"][seg["line"]], seg["k"])  # all segments of a line share k
    assert np.array_equal(seg["rank"][nxt[linked]] * (nxt[linked] != lines["head"][seg["line"][linked]]),
                          (seg["rank"][linked] + 1) * (nxt[linked] != lines["head"][seg["line"][linked]]))
    assert np.array_equal(seg["rank"][lines["head"]], np.zeros(len(lines), np.int32))
    assert np.array_equal(np.bincount(seg["line"], minlength=len(lines)), lines["n_segments"])
    assert np.array_equal(lines["begin"], np.concatenate([[0], np.cumsum(lines["n_segments"] + 1)[:-1]]))
    first_of_line = np.full(len(lines), S, np.int64)
    np.minimum.at(first_of_line, seg["line"], np.arange(S))
    assert np.all(np.diff(first_of_line) > 0)  # numbered by their lowest segment index
    has_prev = np.zeros(S, bool)
    has_prev[nxt[linked]] = True
    for l in lines:
        b, n = int(l["begin"]), int(l["n_segments"])
        if l["closed"]:
            assert vertices[b + n].tobytes() == vertices[b].tobytes() and has_prev[l["head"]] and l["head"] == first_of_line[seg["line"][l["head"]]]
        else:
            assert not has_prev[l["head"]]
    assert info["n_closed"] == int(lines["closed"].sum()) and info["n_longest"] == int(lines["n_segments"].max())
    v = vertices[lines["begin"][seg["line"]] + seg["rank"]]
    assert np.array_equal(v[:, 0].view(np.uint64), seg["x0"].view(np.uint64)) and np.array_equal(v[:, 1].view(np.uint64), seg["y0"].view(np.uint64))


def open_ends_are_on_the_border_or_beside_a_hole(Z, seg, cell_size=1.0, origin=(0, 0)):
    """an end without a next: its vertex lies on the border of the grid of cell centres, or on an edge of a quad with a NaN
    corner (positions in cell units: exact for the unit frame these tests use)"""
    H, W = Z.shape
    nan = np.isnan(Z)
    bad = nan[:-1, :-1] | nan[:-1, 1:] | nan[1:, 1:] | nan[1:, :-1]
    for s in seg[seg["next"] < 0]:
        u, v = s["x1"] / cell_size - 0.5 - origin[0], s["y1"] / cell_size - 0.5 - origin[1]
        if u in (0.0, W - 1.0) or v in (0.0, H - 1.0):
            continue
        if u == np.floor(u):  # on a vertical edge (or a corner): the quads left and right of it
            c, r = int(u), int(np.floor(v))
            near = [(r, c - 1), (r, c)] + ([(r - 1, c - 1), (r - 1, c)] if v == np.floor(v) else [])
        else:
            assert v == np.floor(v)
            r, c = int(v), int(np.floor(u))
            near = [(r - 1, c), (r, c)]
        assert any(0 <= a < H - 1 and 0 <= b < W - 1 and bad[a, b] for a, b in near), (u, v)


def test_noise_known_answer():
    _, Z = noise()
    seg, lines, vertices, info = cr.contours(Z, 0.7, 0.1)
    assert (info["n_segments"], info["n_lines"], info["n_closed"], info["n_longest"]) == (9951, 2189, 868, 57)
    check_invariants(Z, seg, lines, vertices, info)
    open_ends_are_on_the_border_or_beside_a_hole(Z, seg)


def test_cone_known_answer():
    Z = cone()
    seg, lines, vertices, info = cr.contours(Z, 2.5, 0.0)
    assert (info["n_segments"], info["n_lines"]) == (2050, 33)
    closed = sorted(lines["n_segments"][lines["closed"] == 1].tolist(), reverse=True)
    assert closed[:3] == [240, 220, 200] and all(a - b == 20 for a, b in zip(closed, closed[1:]))
    check_invariants(Z, seg, lines, vertices, info)
    open_ends_are_on_the_border_or_beside_a_hole(Z, seg)


def test_exact_plane():
    Z = plane()
    seg, lines, vertices, info = cr.contours(Z, 0.375, 0.125, cell_size=0.5, origin=(-7, 3))
    assert (info["n_segments"], info["n_lines"], info["n_closed"]) == (874, 41, 0)
    check_invariants(Z, seg, lines, vertices, info)
    # every quantity is dyadic: each vertex lies on its level exactly
    for x, y in (("x0", "y0"), ("x1", "y1")):
        u, v = seg[x] / 0.5 - 0.5 + 7, seg[y] / 0.5 - 0.5 - 3
        assert np.array_equal(0.25 * u + 0.5 * v + 3, cr.level(seg["k"], 0.125, 0.375))
    open_ends_are_on_the_border_or_beside_a_hole(Z, seg, 0.5, (-7, 3))


def test_integers_have_zero_length_segments():
    Z = integers()
    seg, lines, vertices, info = cr.contours(Z, 1.0)
    zero = (seg["x0"] == seg["x1"]) & (seg["y0"] == seg["y1"])
    assert zero.sum() > 0 and info["n_segments"] > zero.sum()
    check_invariants(Z, seg, lines, vertices, info)
    open_ends_are_on_the_border_or_beside_a_hole(Z, seg)


def test_multi_level_quad():
    seg, lines, vertices, info = cr.contours(MULTI, 1.0)
    assert info["n_segments"] == 10 and sorted(seg["k"].tolist()) == list(range(1, 11)) and info["k_lo"] == 1 and info["k_hi"] == 10
    check_invariants(MULTI, seg, lines, vertices, info)


@pytest.mark.parametrize("bits,centre_in,Z", CASES, ids=[f"{b:04b}{'' if c is None else '+-'[not c]}" for b, c, _ in CASES])
def test_every_case_of_one_quad(bits, centre_in, Z):
    """the 16 corner cases, and both resolutions of each saddle"""
    seg, lines, vertices, info = cr.contours(Z, 1.0, 0.5)
    inside = [Z[0, 0] >= 0.5, Z[0, 1] >= 0.5, Z[1, 1] >= 0.5, Z[1, 0] >= 0.5]
    assert sum(int(v) << i for i, v in enumerate(inside)) == bits
    k1 = seg[seg["k"] == 0]  # the level 0.5
    assert len(k1) == (0 if bits in (0, 15) else 2 if bits in (5, 10) else 1)
    check_invariants(Z, seg, lines, vertices, info)
    # the edge a vertex lies on, from its position: B y = 0.5, R x = 1.5, T y = 1.5, L x = 0.5
    def edge(x, y):
        return [e for e, on in enumerate((y == 0.5, x == 1.5, y == 1.5, x == 0.5)) if on]
    pairs = [(edge(s["x0"], s["y0"])[0], edge(s["x1"], s["y1"])[0]) for s in k1]
    if bits in (5, 10):
        assert ((((np.float64(Z[0, 0]) + Z[0, 1]) + Z[1, 0]) + Z[1, 1]) * 0.25 >= 0.5) == centre_in
        step = 1 if centre_in else 3
        starts = (0, 2) if bits == 5 else (1, 3)
        assert pairs == [(s, (s + step) & 3) for s in starts]
    elif pairs:
        (s, e), = pairs
        assert inside[s] and not inside[(s + 1) & 3] and not inside[e] and inside[(e + 1) & 3]  # higher ground on the left


def test_holes_only_and_thin_rasters():
    for Z in (np.full((5, 6), np.nan, np.float32), np.zeros((1, 7), np.float32), np.zeros((7, 1), np.float32), np.zeros((1, 1), np.float32)):
        seg, lines, vertices, info = cr.contours(Z, 1.0, 0.5)
        assert len(seg) == len(lines) == len(vertices) == 0 and all(v == 0 for v in info.values())
