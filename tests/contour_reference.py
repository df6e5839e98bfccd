"""The contour-line contract of include/o3dr_contour.h restated in numpy, operation for operation.  Vectorised
per level; the links are made by matching (edge id, k) keys and the lines by walking them on the host, not by the kernels'
index arithmetic or union-find.  numpy's float64 arithmetic rounds every operation and never fuses a multiply-add."""
import numpy as np

CONTOUR_SEGMENT = np.dtype([("x0", "<f8"), ("y0", "<f8"), ("x1", "<f8"), ("y1", "<f8"), ("k", "<i4"), ("line", "<i4"),
                            ("rank", "<i4"), ("next", "<i4")])
CONTOUR_LINE = np.dtype([("head", "<i4"), ("n_segments", "<i4"), ("k", "<i4"), ("closed", "<i4"), ("begin", "<i8"),
                         ("level", "<f8")])
INFO_FIELDS = ("n_quads", "n_quads_crossed", "n_segments", "n_lines", "n_closed", "n_vertices", "n_longest", "k_lo", "k_hi")


def level(k, base, interval):
    """step 1: L_k, the product rounded, then the sum"""
    return np.float64(base) + np.asarray(k).astype(np.float64) * np.float64(interval)


def level_index(z, base, interval):
    """step 1: K(z) of finite float32 values, int64: one division, then the predicate decides"""
    zd = np.asarray(z, np.float32).astype(np.float64)
    k = np.floor((zd - np.float64(base)) / np.float64(interval)).astype(np.int64)
    while True:
        bad = ~(zd >= level(k, base, interval))
        if not bad.any():
            break
        k[bad] -= 1
    while True:
        up = zd >= level(k + 1, base, interval)
        if not up.any():
            break
        k[up] += 1
    return k


def _edge_vertex(Z, horizontal, r, c, lev, cell_size, origin):
    """step 4 on h(r, c) / v(r, c): A = [r, c], B = the cell after it"""
    zA = Z[r, c].astype(np.float64)
    zB = np.where(horizontal, Z[r, np.minimum(c + 1, Z.shape[1] - 1)], Z[np.minimum(r + 1, Z.shape[0] - 1), c]).astype(np.float64)
    t = (lev - zA) / (zB - zA)
    assert np.all((t >= 0) & (t <= 1))
    u = (origin[0] + c).astype(np.float64) + 0.5
    w = (origin[1] + r).astype(np.float64) + 0.5
    x = np.where(horizontal, u + t, u) * np.float64(cell_size)
    y = np.where(horizontal, w, w + t) * np.float64(cell_size)
    return x, y


def contours(Z, interval, base=0.0, cell_size=1.0, origin=(0, 0)):
    """-> segments (CONTOUR_SEGMENT [S]), lines (CONTOUR_LINE [n]), vertices (float64 [S + n, 2]), info (dict of the
    result's counters)"""
    Z = np.ascontiguousarray(Z, np.float32)
    H, W = Z.shape
    assert not np.isinf(Z).any() and interval > 0
    origin = (np.int64(origin[0]), np.int64(origin[1]))
    seg_parts = []  # per (level, start edge): quad, k, order, start edge (horizontal, r, c), end edge (horizontal, r, c)
    info = dict.fromkeys(INFO_FIELDS, 0)
    if H > 1 and W > 1:
        zd = Z.astype(np.float64)
        z = [zd[:-1, :-1], zd[:-1, 1:], zd[1:, 1:], zd[1:, :-1]]  # b0 b1 b2 b3
        valid = ~(np.isnan(z[0]) | np.isnan(z[1]) | np.isnan(z[2]) | np.isnan(z[3]))
        info["n_quads"] = int(valid.sum())
        rr, cc = np.nonzero(valid)
        zq = [v[rr, cc] for v in z]
        crossed = np.zeros(len(rr), bool)
        if len(rr):
            zmin, zmax = np.minimum.reduce(zq), np.maximum.reduce(zq)
            kmin, kmax = level_index(zmin, base, interval), level_index(zmax, base, interval)
            assert np.abs(kmin).max() <= 2 ** 30 and np.abs(kmax).max() <= 2 ** 30
            # the edges of quad (r, c) in the order B R T L: (horizontal, dr, dc)
            edges = [(True, 0, 0), (False, 0, 1), (True, 1, 0), (False, 0, 0)]
            for k in range(int(kmin.min()) + 1, int(kmax.max()) + 1):
                act = np.nonzero((kmin < k) & (k <= kmax))[0]
                if not len(act):
                    continue
                crossed[act] = True
                lev = level(np.int64(k), base, interval)
                inside = [zq[i][act] >= lev for i in range(4)]
                start = [inside[e] & ~inside[(e + 1) & 3] for e in range(4)]
                end = [~inside[e] & inside[(e + 1) & 3] for e in range(4)]
                n_start = sum(s.astype(np.int64) for s in start)
                assert np.all((n_start >= 1) & (n_start <= 2)) and np.all(n_start == sum(e.astype(np.int64) for e in end))
                saddle = n_start == 2
                centre = (((zq[0][act] + zq[1][act]) + zq[3][act]) + zq[2][act]) * 0.25
                centre_in = centre >= lev
                the_end = np.zeros(len(act), np.int64)
                for e in range(4):
                    the_end[end[e] & ~saddle] = e
                for s in range(4):
                    m = np.nonzero(start[s])[0]
                    if not len(m):
                        continue
                    e = np.where(saddle[m], np.where(centre_in[m], (s + 1) & 3, (s + 3) & 3), the_end[m])
                    r, c = rr[act[m]], cc[act[m]]
                    eh = np.array([edges[i][0] for i in range(4)])[e]
                    er = r + np.array([edges[i][1] for i in range(4)])[e]
                    ec = c + np.array([edges[i][2] for i in range(4)])[e]
                    n = len(m)
                    seg_parts.append((r * (W - 1) + c, np.full(n, k, np.int64), np.full(n, s, np.int64),
                                      np.full(n, edges[s][0]), r + edges[s][1], c + edges[s][2], eh, er, ec))
        info["n_quads_crossed"] = int(crossed.sum())
    if not seg_parts:
        return np.zeros(0, CONTOUR_SEGMENT), np.zeros(0, CONTOUR_LINE), np.zeros((0, 2), np.float64), info
    quad, k, order, sh, sr, sc, eh, er, ec = (np.concatenate([p[i] for p in seg_parts]) for i in range(9))
    o = np.lexsort((order, k, quad))  # step 3: by quad, then k, then the start edge
    quad, k, order, sh, sr, sc, eh, er, ec = (v[o] for v in (quad, k, order, sh, sr, sc, eh, er, ec))
    S = len(quad)
    lev = level(k, base, interval)
    seg = np.zeros(S, CONTOUR_SEGMENT)
    seg["x0"], seg["y0"] = _edge_vertex(Z, sh, sr, sc, lev, cell_size, origin)
    seg["x1"], seg["y1"] = _edge_vertex(Z, eh, er, ec, lev, cell_size, origin)
    seg["k"] = k
    # step 5: a start crossing (edge, k) belongs to one segment; next = the segment that starts where this one ends
    k0, nk = int(k.min()), int(k.max()) - int(k.min()) + 1
    start_key = ((~sh).astype(np.int64) * H * W + sr * W + sc) * nk + (k - k0)
    end_key = ((~eh).astype(np.int64) * H * W + er * W + ec) * nk + (k - k0)
    by_key = np.argsort(start_key, kind="stable")
    sorted_keys = start_key[by_key]
    assert np.all(sorted_keys[1:] != sorted_keys[:-1])
    pos = np.minimum(np.searchsorted(sorted_keys, end_key), S - 1)
    nxt = np.where(sorted_keys[pos] == end_key, by_key[pos], -1).astype(np.int64)
    seg["next"] = nxt
    # step 6: walk the lines
    prev = np.full(S, -1, np.int64)
    linked = np.nonzero(nxt >= 0)[0]
    assert len(np.unique(nxt[linked])) == len(linked)  # prev is a function
    prev[nxt[linked]] = linked
    visited = np.zeros(S, bool)
    found = []  # (lowest index, head, closed, members in rank order)
    nx = nxt.tolist()
    for closed, heads in ((0, np.nonzero(prev < 0)[0].tolist()), (1, range(S))):
        for h in heads:
            if visited[h]:
                continue
            members, i = [], h
            while i >= 0 and not visited[i]:
                visited[i] = True
                members.append(i)
                i = nx[i]
            assert (i == h) if closed else (i < 0)
            found.append((min(members), h, closed, members))
    found.sort(key=lambda f: f[0])
    lines = np.zeros(len(found), CONTOUR_LINE)
    vertices = np.zeros((S + len(found), 2), np.float64)
    begin = 0
    for number, (_, h, closed, members) in enumerate(found):
        m = np.array(members)
        seg["line"][m] = number
        seg["rank"][m] = np.arange(len(m))
        lines[number] = (h, len(m), k[h], closed, begin, level(k[h], base, interval))
        vertices[begin:begin + len(m), 0], vertices[begin:begin + len(m), 1] = seg["x0"][m], seg["y0"][m]
        vertices[begin + len(m)] = (seg["x1"][m[-1]], seg["y1"][m[-1]])
        begin += len(m) + 1
    info.update(n_segments=S, n_lines=len(found), n_closed=int(lines["closed"].sum()), n_vertices=S + len(found),
                n_longest=int(lines["n_segments"].max()), k_lo=int(k.min()), k_hi=int(k.max()))
    return seg, lines, vertices, info
