// Stand-alone check of online_3d_reconstruction_amd/csrc/o3dr_image_stack.h, built and run by test_image_stack_host.py with
// -fsanitize=address,undefined -fno-sanitize-recover=all: every CHECK that fails, and any report of a sanitizer, ends the
// program with a non-zero status.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "o3dr_image_stack.h"

using namespace o3dr;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                     \
        }                                                                \
    } while (0)

static bool is(const char* got, const char* want) { return got && !strcmp(got, want); }

static ImageStack stack(int64_t fs, int64_t pitch, int32_t rows, int32_t cols, int32_t n_frames, int32_t px, const void* ptr = nullptr)
{
    return ImageStack{ptr, fs, pitch, rows, cols, n_frames, px};
}

// the extent of a stack that must have one
static int64_t extent(const ImageStack& s)
{
    int64_t bytes = -1;
    CHECK(stack_extent(s, &bytes) == nullptr);
    return bytes;
}
static bool overflows(const ImageStack& s)
{
    int64_t bytes = -1;
    return is(stack_extent(s, &bytes), "image stack extent overflows int64");
}

int main()
{
    const int64_t kMax = INT64_MAX, k62 = (int64_t)1 << 62;

    // ---- extent: 9 x 33 x 2 frames against the formula written out by hand ----
    CHECK(extent(stack(9 * 33, 33, 9, 33, 2, 1)) == 297 + 264 + 33);     // tight: all 594 bytes
    CHECK(extent(stack(9 * 66, 66, 9, 33, 2, 2)) == 594 + 528 + 66);     // 1188
    CHECK(extent(stack(9 * 264, 264, 9, 33, 2, 8)) == 2376 + 2112 + 264);  // 4752
    // padded pitch and stride: the padding behind the last row and the last frame is not part of it
    CHECK(extent(stack(1000, 40, 9, 33, 2, 1)) == 1000 + 8 * 40 + 33);
    CHECK(extent(stack(1000, 100, 9, 33, 2, 3)) == 1000 + 8 * 100 + 99);
    CHECK(extent(stack(5000, 300, 9, 33, 3, 8)) == 2 * 5000 + 8 * 300 + 264);
    // one frame: the stride is not read, whatever it holds
    CHECK(extent(stack(kMax, 40, 9, 33, 1, 1)) == 8 * 40 + 33);
    CHECK(extent(stack(INT64_MIN, 40, 9, 33, 1, 1)) == 8 * 40 + 33);
    CHECK(extent(stack(-12345, 33, 1, 33, 1, 1)) == 33);

    // ---- extent: overflow is reported, not computed ----
    CHECK(overflows(stack(kMax, 33, 9, 33, 2, 1)));
    CHECK(overflows(stack(k62, 33, 9, 33, 5, 1)));
    CHECK(overflows(stack(0, k62, 8192, 33, 1, 1)));
    CHECK(overflows(stack(k62, k62, 2, 33, 2, 1)));  // each product fits, their sum does not
    {  // the largest stack that still fits, and the one a byte larger
        const int64_t rest = 8 * 40 + 33;
        CHECK(extent(stack(kMax - rest, 40, 9, 33, 2, 1)) == kMax);
        CHECK(overflows(stack(kMax - rest + 1, 40, 9, 33, 2, 1)));
        CHECK(extent(stack(0, (kMax - 33) / 8191, 8192, 33, 1, 1)) == (kMax - 33) / 8191 * 8191 + 33);
    }

    // ---- sides ----
    CHECK(stack_sides_error(1, 1, 8192) == nullptr && stack_sides_error(8192, 8192, 8192) == nullptr);
    const int32_t bad_sides[] = {0, -1, 8193, INT32_MIN, INT32_MAX};
    for (int32_t bad : bad_sides) {
        CHECK(is(stack_sides_error(bad, 33, 8192), "rows and cols must be in 1..8192"));
        CHECK(is(stack_sides_error(9, bad, 8192), "rows and cols must be in 1..8192"));
    }
    CHECK(stack_pixels(9, 33, 2, 8192) == 594 && stack_pixels(9, 33, 0, 8192) == 0 && stack_pixels(8192, 8192, 3, 8192) == (int64_t)3 << 26);
    CHECK(stack_pixels(0, 33, 2, 8192) == 0 && stack_pixels(9, 8193, 2, 8192) == 0 && stack_pixels(9, 33, -1, 8192) == 0);

    // ---- layout ----
    CHECK(stack_layout_error(stack(297, 33, 9, 33, 2, 1)) == nullptr);
    CHECK(stack_layout_error(stack(1000, 100, 9, 33, 2, 3)) == nullptr);
    CHECK(is(stack_layout_error(stack(297, 32, 9, 33, 2, 1)), "pitch smaller than a row"));
    CHECK(is(stack_layout_error(stack(2376, 263, 9, 33, 2, 8)), "pitch smaller than a row"));
    CHECK(is(stack_layout_error(stack(297, 0, 9, 33, 2, 1)), "pitch smaller than a row"));
    CHECK(is(stack_layout_error(stack(297, -33, 9, 33, 2, 1)), "pitch smaller than a row"));
    CHECK(is(stack_layout_error(stack(296, 33, 9, 33, 2, 1)), "frame stride smaller than a frame"));
    CHECK(is(stack_layout_error(stack(899, 100, 9, 33, 2, 3)), "frame stride smaller than a frame"));
    CHECK(stack_layout_error(stack(900, 100, 9, 33, 2, 3)) == nullptr);
    CHECK(is(stack_layout_error(stack(0, 33, 9, 33, 2, 1)), "frame stride smaller than a frame"));
    CHECK(is(stack_layout_error(stack(-1, 33, 9, 33, 2, 1)), "frame stride smaller than a frame"));
    CHECK(stack_layout_error(stack(-1, 33, 9, 33, 1, 1)) == nullptr);  // one frame: the stride is not read
    CHECK(is(stack_layout_error(stack(kMax, k62, 8192, 33, 2, 1)), "frame stride smaller than a frame"));  // rows * pitch is beyond int64
    CHECK(stack_layout_error(stack(kMax, kMax / 8192, 8192, 33, 2, 1)) == nullptr);
    // alignment to an element size
    alignas(8) static char buf[64];
    CHECK(stack_aligned(stack(600, 66, 9, 33, 2, 2, buf), 2) && stack_aligned(stack(601, 67, 9, 33, 2, 1, buf + 1), 1));
    CHECK(!stack_aligned(stack(600, 66, 9, 33, 2, 2, buf + 1), 2) && !stack_aligned(stack(600, 67, 9, 33, 2, 2, buf), 2));
    CHECK(!stack_aligned(stack(601, 66, 9, 33, 2, 2, buf), 2) && stack_aligned(stack(601, 66, 9, 33, 1, 2, buf), 2));
    CHECK(stack_aligned(stack(2400, 264, 9, 33, 2, 8, buf + 8), 8) && !stack_aligned(stack(2400, 264, 9, 33, 2, 8, buf + 4), 8));
    CHECK(!stack_aligned(stack(2404, 264, 9, 33, 2, 8, buf), 8) && !stack_aligned(stack(2400, 268, 9, 33, 2, 8, buf), 8));

    // ---- overlap of two byte ranges, in both orders ----
    CHECK(!ranges_overlap(buf, 16, buf + 16, 16) && !ranges_overlap(buf + 16, 16, buf, 16));  // touching
    CHECK(ranges_overlap(buf, 17, buf + 16, 16) && ranges_overlap(buf + 16, 16, buf, 17));    // one shared byte
    CHECK(ranges_overlap(buf, 64, buf + 8, 8) && ranges_overlap(buf + 8, 8, buf, 64));        // one inside the other
    CHECK(ranges_overlap(buf, 16, buf, 16));
    CHECK(!ranges_overlap(buf, 8, buf + 32, 8) && !ranges_overlap(buf + 32, 8, buf, 8));      // apart

    // ---- frames per launch group ----
    const size_t GiB = (size_t)1 << 30;
    CHECK(frames_per_group(GiB, 2 * GiB, 7, 0) == 1);  // a budget below one frame: one frame still forms a group
    CHECK(frames_per_group(GiB, GiB / 4, 7, 0) == 4 && frames_per_group(GiB, GiB / 4 + 1, 7, 0) == 3);
    CHECK(frames_per_group(GiB, 1000, 7, 0) == 7);     // group_frames 0: no bound of the caller's
    CHECK(frames_per_group(GiB, 1000, 7, 3) == 3 && frames_per_group(GiB, 1000, 2, 3) == 2 && frames_per_group(GiB, GiB / 2, 7, 3) == 2);
    CHECK(frames_per_group(GiB, 1000, 40000, 0) == 32768 && frames_per_group(SIZE_MAX, 1, 40000, 0) == 32768);
    CHECK(frames_per_group(GiB, 1000, 40000, 33000) == 32768 && frames_per_group(GiB, 1000, 32768, 0) == 32768);
    CHECK(frames_per_group(SIZE_MAX, 8, 5, 0) == 5);

    puts("image stack: ok");
    return 0;
}
