/* o3dr_contour.h - contour lines of a float32 elevation raster (libo3dr.so; o3dr.h holds the context, the error codes, the
 * memory kinds and the map raster whose frame this header uses; o3dr_dem.h the operators that make a hole-free raster). */
#ifndef O3DR_CONTOUR_H
#define O3DR_CONTOUR_H
#include "o3dr.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- contour lines: the level curves of a float32 raster as linked segments, lines and polyline vertices (marching
 * squares over the quads of four cell centres).  The reference has no such tool; the contract is
 * this library's own.  Everything but the vertices is integer topology, and a vertex is a fixed sequence of fp64
 * operations, each correctly rounded, on the two values of its edge: results are bit-identical across calls, memory
 * kinds and whatever tiling computes them.
 *
 * Input: `raster`, row-major float32 [height, width].  A NaN of any payload is a hole; every other value must be finite.
 * Element [r, c] is the value at the CENTRE of cell (cx0 + c, cy0 + r) of a frame with cell_size: a position c + t along a
 * row has the map coordinate x = (((double)(cx0 + c) + 0.5) + t) * cell_size, and y likewise from cy0 + r.  `(double)z`
 * below is the float converted, which is exact.
 *   1. Levels: L_k = base + (double)k * interval for integer k (the product rounded, then the sum; no fused multiply-add).
 *      z is inside level k iff (double)z >= L_k, which is monotone in k.  K(z) = the greatest k with z inside: found with
 *      one division and a correction loop, defined by the predicate.  K of the raster's least and greatest value must lie
 *      within +-2^30.
 *   2. Quads: quad (r, c), 0 <= r < height - 1, 0 <= c < width - 1, has the corners b0 = [r, c], b1 = [r, c + 1],
 *      b2 = [r + 1, c + 1], b3 = [r + 1, c] (counter-clockwise with x to the right and y = rows upward) and the edges, in
 *      that order, B: b0 -> b1 = h(r, c), R: b1 -> b2 = v(r, c + 1), T: b2 -> b3 = h(r + 1, c), L: b3 -> b0 = v(r, c).  A
 *      quad with a NaN corner emits nothing; another one emits the segments of every k in K(min corner) + 1 .. K(max
 *      corner), ascending.
 *   3. Segments of level k in a quad: an edge whose first corner (in the order above) is inside and whose second is outside
 *      is a start, the reverse an end.  One start and one end: the segment runs from the start to the end, higher ground
 *      on its left.  Two of each (a saddle): with c = (((z0 + z1) + z3) + z2) * 0.25 in fp64, c inside L_k joins every
 *      start to the next end counter-clockwise after it (B -> R, T -> L, R -> T, L -> B), else to the end before it
 *      (B -> L, T -> R, R -> B, L -> T); the two segments in the order of their start edges B, R, T, L.  Segment order: by
 *      quad index r * (width - 1) + c, then k, then that start-edge order.
 *   4. Vertices: the crossing of level k on an edge is computed from the edge, not the quad: A = the edge's corner with the
 *      lower (r, c), B the other; t = (L_k - zA) / (zB - zA) in fp64 (the denominator is never 0, 0 <= t <= 1).  On
 *      h(r, c): x = (((double)(cx0 + c) + 0.5) + t) * cell_size, y = ((double)(cy0 + r) + 0.5) * cell_size; on v(r, c): y
 *      = (((double)(cy0 + r) + 0.5) + t) * cell_size, x = ((double)(cx0 + c) + 0.5) * cell_size.  The two quads that share
 *      an edge produce the same bits.  A level equal to a corner value gives t = 0 or 1 and may give zero-length
 *      segments: both are valid.
 *   5. Links: next[i] = the segment of the same k whose start edge is i's end edge, or -1 (the end lies on the raster's
 *      border or beside a quad with a NaN corner).  A start crossing (edge, k) belongs to exactly one segment: next is a
 *      function and so is its inverse.
 *   6. Lines: a line is a connected component of next.  An open line's head is its segment without a predecessor; a
 *      closed line (closed = 1) has none and its head is its lowest segment index.  rank is 0 at the head and grows along
 *      next.  Lines are numbered 0 .. n_lines - 1 in ascending order of their lowest segment index; begin = the exclusive
 *      sum of n_segments + 1 over the lines in that order.  vertices[begin + rank] is a segment's start, vertices[begin +
 *      n_segments] the end of the line's last segment: on a closed line bitwise the first vertex.
 *   7. Result: n_quads = the quads without a NaN corner, n_quads_crossed those that emit; k_lo / k_hi = the least and the
 *      greatest k emitted (both 0 when nothing is); n_vertices = n_segments + n_lines; n_longest = the segments of the
 *      longest line.
 * o3dr_raster_contours_count runs the count pass and its sum only.  o3dr_raster_contours: any pointer of `outputs` may be
 * NULL; n_lines <= n_segments and n_vertices <= 2 * n_segments are the bounds a caller sizes by.  If a capacity is below
 * what a non-NULL output needs, the call returns O3DR_ERR_CAPACITY with *result set and nothing else written; above
 * O3DR_CONTOUR_MAX_SEGMENTS segments it returns O3DR_ERR_CAPACITY with n_segments set.
 * Errors, O3DR_ERR_INVALID_ARG, in this order: a NULL argument; a bad mem; width or height < 1; interval or base not
 * finite, or interval <= 0; cell_size not finite, or <= 0; more than O3DR_RASTER_MAX_CELLS cells; an infinite input value;
 * the +-2^30 level range.  On an error the host outputs and the result are zeroed.  A raster of one row or one column has
 * no quad: zero segments, no error.  The call synchronises and reuses the operators' scratch: cloud_big and the sort
 * workspace are left alone. */
#define O3DR_CONTOUR_MAX_SEGMENTS (1 << 28)
typedef struct o3dr_contour_params {
    int32_t width, height;  /* no default (0 x 0 is rejected) */
    double interval;        /* no default: the caller sets it, > 0 */
    double base;            /* 0.0 */
    double cell_size;       /* 1.0 */
    int32_t cx0, cy0;       /* 0, 0: the frame's cell of element [0, 0] */
} o3dr_contour_params;
typedef struct o3dr_contour_segment {  /* 48 bytes */
    double x0, y0, x1, y1;
    int32_t k, line, rank, next;
} o3dr_contour_segment;
typedef struct o3dr_contour_line {  /* 32 bytes */
    int32_t head, n_segments, k, closed;
    int64_t begin;
    double level;  /* L_k */
} o3dr_contour_line;
typedef struct o3dr_contour_outputs {
    o3dr_contour_segment* segments;  /* may be NULL */
    int64_t seg_capacity;
    o3dr_contour_line* lines;        /* may be NULL */
    int64_t line_capacity;
    double* vertices;                /* [n_vertices][2], may be NULL */
    int64_t vertex_capacity;         /* in vertices */
} o3dr_contour_outputs;
typedef struct o3dr_contour_result {
    int64_t n_quads, n_quads_crossed, n_segments, n_lines, n_closed, n_vertices, n_longest;
    int32_t k_lo, k_hi;
} o3dr_contour_result;
void o3dr_contour_default_params(o3dr_contour_params* p);
int  o3dr_raster_contours_count(o3dr_ctx* ctx, const float* raster, const o3dr_contour_params* p, int64_t* n_segments,
                                int32_t mem);
int  o3dr_raster_contours(o3dr_ctx* ctx, const float* raster, const o3dr_contour_params* p, const o3dr_contour_outputs* out,
                          o3dr_contour_result* res, int32_t mem);

#ifdef __cplusplus
}
#endif
#endif
