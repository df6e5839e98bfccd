// o3dr_image_stack.h — what a valid image stack is and how many bytes it spans.
//
// The image operators (ORB, rectification, stereo, the disparity filter, the multi-view filter, segmentation) take
// n_frames images of rows x cols pixels of px bytes, rows `pitch` bytes apart and frames `fs` bytes apart, in host or
// device memory.  Host only and free of HIP, of o3dr_ctx and of globals: every function is pure, and a check returns the
// text for o3dr_last_error() (nullptr: fine), which the caller hands to fail(O3DR_ERR_INVALID_ARG, ...).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace o3dr {

struct ImageStack {
    const void* ptr;
    int64_t fs, pitch;  // bytes between frames (not read where n_frames is 1) and between rows
    int32_t rows, cols, n_frames;
    int32_t px;  // bytes per pixel: channels of a uint8 image, the element size of a disparity image
};

// a side within 1..max_side (the operator's O3DR_*_MAX_SIDE of include/o3dr.h)
inline bool stack_side_ok(int32_t v, int32_t max_side) { return v >= 1 && v <= max_side; }
inline const char* stack_sides_error(int32_t rows, int32_t cols, int32_t max_side)
{
    return stack_side_ok(rows, max_side) && stack_side_ok(cols, max_side) ? nullptr : "rows and cols must be in 1..8192";
}
// n_frames * rows * cols where all three are within their limits, else 0: the entry points know their outputs' sizes
// only there
inline int64_t stack_pixels(int32_t rows, int32_t cols, int32_t n_frames, int32_t max_side)
{
    return stack_side_ok(rows, max_side) && stack_side_ok(cols, max_side) && n_frames >= 0 ? (int64_t)n_frames * rows * cols : 0;
}

// rows do not overlap, frames do not overlap (sides within their limits; no product here can overflow)
inline const char* stack_layout_error(const ImageStack& s)
{
    if (s.pitch < (int64_t)s.cols * s.px) return "pitch smaller than a row";
    if (s.n_frames > 1 && s.fs / s.rows < s.pitch) return "frame stride smaller than a frame";  // fs < rows * pitch
    return nullptr;
}
// pointer, pitch and (where it is read) frame stride are multiples of `elem` bytes
inline bool stack_aligned(const ImageStack& s, int64_t elem)
{
    return (uintptr_t)s.ptr % (uintptr_t)elem == 0 && s.pitch % elem == 0 && (s.n_frames <= 1 || s.fs % elem == 0);
}

// *bytes = from the first byte of the stack to one past its last: fs (n_frames - 1) + pitch (rows - 1) + cols px, for a
// stack of at least one frame that passed the checks above.  An extent beyond int64_t is an error, found without
// computing it.
inline const char* stack_extent(const ImageStack& s, int64_t* bytes)
{
    int64_t frames = 0, rows = 0, sum = 0;
    if ((s.n_frames > 1 && __builtin_mul_overflow(s.fs, (int64_t)(s.n_frames - 1), &frames)) ||
        __builtin_mul_overflow(s.pitch, (int64_t)(s.rows - 1), &rows) || __builtin_add_overflow(frames, rows, &sum) ||
        __builtin_add_overflow(sum, (int64_t)s.cols * s.px, bytes))
        return "image stack extent overflows int64";
    return nullptr;
}

// do the byte ranges [a, a + a_bytes) and [b, b + b_bytes) share a byte (in either memory kind)
inline bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// frames per launch group: what `budget` bytes of scratch hold at per_frame bytes each (at least one frame), no more than
// the stack has, than a launch's 32768, and than the caller's group_frames where that is positive
inline size_t frames_per_group(size_t budget, size_t per_frame, int32_t n_frames, int32_t group_frames)
{
    size_t group = budget / per_frame;
    if (group < 1) group = 1;
    if (group > (size_t)n_frames) group = (size_t)n_frames;
    if (group > 32768) group = 32768;
    if (group_frames > 0 && group > (size_t)group_frames) group = (size_t)group_frames;
    return group;
}

}  // namespace o3dr
