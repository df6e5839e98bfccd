// png_io.cpp — minimal PNG reader (zlib inflate + PNG unfiltering) standing in for the two cv::imread
// calls on the hot path's input side (pose_functions.cpp:526 colour, :548 IMREAD_GRAYSCALE).
// 8-bit, non-interlaced, colour types 0/2/3/4/6 — what the reference's bundled data uses.  read_png_labels reads the
// segment label images of --use_segment_labels: greyscale, 8 or 16 bits, non-interlaced.  write_png_grey8 writes the
// disparity image of --stereo_disparity, write_png_bgr8 the colour images of --rectify_pair, write_png_grey16 the label
// image of --segment_image: 8 (16: big-endian) bits a sample, filter 0, stored (uncompressed) deflate blocks.
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "o3dr_host.h"

namespace o3dr_host {

static uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
static int paeth(int a, int b, int c)
{
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

Image8 read_png(const std::string& path, bool grayscale)
{
    Image8 out;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return out;
    std::vector<uint8_t> file;
    uint8_t buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) file.insert(file.end(), buf, buf + n);
    fclose(f);
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    if (file.size() < 33 || memcmp(file.data(), sig, 8) != 0) return out;
    uint32_t w = 0, h = 0;
    int depth = 0, ctype = 0, interlace = 0;
    std::vector<uint8_t> idat, plte;
    for (size_t pos = 8; pos + 12 <= file.size();) {
        const uint32_t len = be32(&file[pos]);
        const uint8_t* type = &file[pos + 4];
        const uint8_t* data = &file[pos + 8];
        if (pos + 12 + len > file.size()) return out;
        if (!memcmp(type, "IHDR", 4)) {
            w = be32(data);
            h = be32(data + 4);
            depth = data[8];
            ctype = data[9];
            interlace = data[12];
        } else if (!memcmp(type, "PLTE", 4)) {
            plte.assign(data, data + len);
        } else if (!memcmp(type, "IDAT", 4)) {
            idat.insert(idat.end(), data, data + len);
        } else if (!memcmp(type, "IEND", 4)) {
            break;
        }
        pos += 12 + len;
    }
    if (!w || !h || depth != 8 || interlace != 0) return out;
    int spp;  // samples per pixel in the file
    switch (ctype) {
        case 0: spp = 1; break;
        case 2: spp = 3; break;
        case 3: spp = 1; break;
        case 4: spp = 2; break;
        case 6: spp = 4; break;
        default: return out;
    }
    const size_t stride = (size_t)w * spp;
    std::vector<uint8_t> raw((stride + 1) * h);
    uLongf raw_len = (uLongf)raw.size();
    if (uncompress(raw.data(), &raw_len, idat.data(), (uLong)idat.size()) != Z_OK || raw_len != raw.size()) return out;
    std::vector<uint8_t> img(stride * h);
    for (uint32_t y = 0; y < h; ++y) {
        const uint8_t ft = raw[(stride + 1) * y];
        const uint8_t* src = &raw[(stride + 1) * y + 1];
        uint8_t* cur = &img[stride * y];
        const uint8_t* up = y ? &img[stride * (y - 1)] : nullptr;
        for (size_t i = 0; i < stride; ++i) {
            const int a = i >= (size_t)spp ? cur[i - spp] : 0, b = up ? up[i] : 0, c = (up && i >= (size_t)spp) ? up[i - spp] : 0;
            int v = src[i];
            switch (ft) {
                case 0: break;
                case 1: v += a; break;
                case 2: v += b; break;
                case 3: v += (a + b) >> 1; break;
                case 4: v += paeth(a, b, c); break;
                default: return out;
            }
            cur[i] = (uint8_t)v;
        }
    }
    out.rows = (int)h;
    out.cols = (int)w;
    out.channels = grayscale ? 1 : 3;
    out.data.resize((size_t)w * h * out.channels);
    for (size_t p = 0; p < (size_t)w * h; ++p) {
        uint8_t r, g, b;
        const uint8_t* s = &img[p * spp];
        if (ctype == 0 || ctype == 4) {
            r = g = b = s[0];
        } else if (ctype == 3) {
            if ((size_t)s[0] * 3 + 2 >= plte.size()) { out = Image8(); return out; }
            r = plte[s[0] * 3]; g = plte[s[0] * 3 + 1]; b = plte[s[0] * 3 + 2];
        } else {
            r = s[0]; g = s[1]; b = s[2];
        }
        if (grayscale) {
            // grey files pass through unchanged (the disparity PNGs are 8-bit grey); colour input is
            // reduced with OpenCV's fixed-point BT.601 weights — not bit-pinned against libpng's own path
            out.data[p] = (r == g && g == b) ? r : (uint8_t)((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14);
        } else {
            out.data[p * 3] = b;  // cv::imread delivers B,G,R
            out.data[p * 3 + 1] = g;
            out.data[p * 3 + 2] = r;
        }
    }
    return out;
}

// Segment labels: colour type 0 at 8 or 16 bits per sample (big-endian in the file).  A reader of its own: read_png stays
// what it is.
Image16 read_png_labels(const std::string& path)
{
    Image16 out;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return out;
    std::vector<uint8_t> file;
    uint8_t buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) file.insert(file.end(), buf, buf + n);
    fclose(f);
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    if (file.size() < 33 || memcmp(file.data(), sig, 8) != 0) return out;
    uint32_t w = 0, h = 0;
    int depth = 0, ctype = -1, interlace = 0;
    std::vector<uint8_t> idat;
    for (size_t pos = 8; pos + 12 <= file.size();) {
        const uint32_t len = be32(&file[pos]);
        const uint8_t* type = &file[pos + 4];
        const uint8_t* data = &file[pos + 8];
        if (pos + 12 + (size_t)len > file.size()) return out;
        if (!memcmp(type, "IHDR", 4)) {
            if (len < 13) return out;
            w = be32(data);
            h = be32(data + 4);
            depth = data[8];
            ctype = data[9];
            interlace = data[12];
        } else if (!memcmp(type, "IDAT", 4)) {
            idat.insert(idat.end(), data, data + len);
        } else if (!memcmp(type, "IEND", 4)) {
            break;
        }
        pos += 12 + (size_t)len;
    }
    if (!w || !h || w > 65536 || h > 65536 || ctype != 0 || (depth != 8 && depth != 16) || interlace != 0) return out;
    const size_t bpp = (size_t)depth / 8, stride = (size_t)w * bpp;
    std::vector<uint8_t> raw((stride + 1) * h);
    uLongf raw_len = (uLongf)raw.size();
    if (uncompress(raw.data(), &raw_len, idat.data(), (uLong)idat.size()) != Z_OK || raw_len != raw.size()) return out;
    std::vector<uint8_t> img(stride * h);
    for (uint32_t y = 0; y < h; ++y) {
        const uint8_t ft = raw[(stride + 1) * y];
        const uint8_t* src = &raw[(stride + 1) * y + 1];
        uint8_t* cur = &img[stride * y];
        const uint8_t* up = y ? &img[stride * (y - 1)] : nullptr;
        for (size_t i = 0; i < stride; ++i) {
            const int a = i >= bpp ? cur[i - bpp] : 0, b = up ? up[i] : 0, c = (up && i >= bpp) ? up[i - bpp] : 0;
            int v = src[i];
            switch (ft) {
                case 0: break;
                case 1: v += a; break;
                case 2: v += b; break;
                case 3: v += (a + b) >> 1; break;
                case 4: v += paeth(a, b, c); break;
                default: return out;
            }
            cur[i] = (uint8_t)v;
        }
    }
    out.rows = (int)h;
    out.cols = (int)w;
    out.data.resize((size_t)w * h);
    for (size_t p = 0; p < (size_t)w * h; ++p)
        out.data[p] = bpp == 2 ? (uint16_t)((img[2 * p] << 8) | img[2 * p + 1]) : (uint16_t)img[p];
    return out;
}

// 8-bit writers: every row with filter type 0, the zlib stream made of stored blocks (no compression), so the
// only arithmetic is the two checksums.  Any PNG reader takes it, read_png above included.
static uint32_t crc32_png(const uint8_t* p, size_t n, uint32_t crc)
{
    static uint32_t table[256];
    if (!table[1])
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            table[i] = c;
        }
    crc = ~crc;
    for (size_t i = 0; i < n; ++i) crc = table[(crc ^ p[i]) & 0xFF] ^ (crc >> 8);
    return ~crc;
}
static void put_be32(std::vector<uint8_t>& v, uint32_t x)
{
    for (int s = 24; s >= 0; s -= 8) v.push_back((uint8_t)(x >> s));
}
static void put_chunk(std::vector<uint8_t>& file, const char* type, const std::vector<uint8_t>& data)
{
    put_be32(file, (uint32_t)data.size());
    const size_t start = file.size();
    file.insert(file.end(), type, type + 4);
    file.insert(file.end(), data.begin(), data.end());
    put_be32(file, crc32_png(&file[start], file.size() - start, 0));
}
// `raw`: every row as its filter byte (0) and its samples; colour_type 0 (grey) or 2 (R G B)
static bool write_png_rows(const std::string& path, const std::vector<uint8_t>& raw, int rows, int cols, uint8_t colour_type,
                           uint8_t depth = 8)
{
    std::vector<uint8_t> z = {0x78, 0x01};  // zlib header: deflate, 32 KiB window, no preset dictionary
    uint32_t a = 1, b = 0;                  // Adler-32 of the raw bytes
    for (size_t pos = 0; pos < raw.size();) {
        const size_t n = raw.size() - pos < 65535 ? raw.size() - pos : 65535;
        z.push_back(pos + n == raw.size() ? 1 : 0);  // BFINAL, BTYPE = 00 (stored)
        z.push_back((uint8_t)(n & 0xFF));
        z.push_back((uint8_t)(n >> 8));
        z.push_back((uint8_t)(~n & 0xFF));
        z.push_back((uint8_t)((~n >> 8) & 0xFF));
        z.insert(z.end(), raw.begin() + (long)pos, raw.begin() + (long)(pos + n));
        for (size_t i = pos; i < pos + n; ++i) {
            a = (a + raw[i]) % 65521u;
            b = (b + a) % 65521u;
        }
        pos += n;
    }
    put_be32(z, (b << 16) | a);
    std::vector<uint8_t> file = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a}, ihdr;
    put_be32(ihdr, (uint32_t)cols);
    put_be32(ihdr, (uint32_t)rows);
    const uint8_t tail[5] = {depth, colour_type, 0, 0, 0};  // bit depth, colour type, deflate, adaptive filtering, no interlace
    ihdr.insert(ihdr.end(), tail, tail + 5);
    put_chunk(file, "IHDR", ihdr);
    put_chunk(file, "IDAT", z);
    put_chunk(file, "IEND", {});
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(file.data(), 1, file.size(), f) == file.size();
    return fclose(f) == 0 && ok;
}
bool write_png_grey8(const std::string& path, const uint8_t* data, int rows, int cols)
{
    if (!data || rows < 1 || cols < 1) return false;
    std::vector<uint8_t> raw(((size_t)cols + 1) * rows);  // filter byte 0 + the row
    for (int y = 0; y < rows; ++y) memcpy(&raw[((size_t)cols + 1) * y + 1], data + (size_t)cols * y, (size_t)cols);
    return write_png_rows(path, raw, rows, cols, 0);
}
// 16 bits per sample, big-endian in the file: a segment label image, what read_png_labels reads
bool write_png_grey16(const std::string& path, const uint16_t* data, int rows, int cols)
{
    if (!data || rows < 1 || cols < 1) return false;
    const size_t stride = (size_t)cols * 2 + 1;
    std::vector<uint8_t> raw(stride * rows);  // filter byte 0 + the row
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols; ++x) {
            const uint16_t v = data[(size_t)cols * y + x];
            raw[stride * y + 1 + (size_t)x * 2] = (uint8_t)(v >> 8);
            raw[stride * y + 2 + (size_t)x * 2] = (uint8_t)(v & 0xFF);
        }
    return write_png_rows(path, raw, rows, cols, 0, 16);
}
// the same for an interleaved B G R image (cv::imwrite's view of a CV_8UC3 Mat): the file holds R G B
bool write_png_bgr8(const std::string& path, const uint8_t* data, int rows, int cols)
{
    if (!data || rows < 1 || cols < 1) return false;
    const size_t stride = (size_t)cols * 3 + 1;
    std::vector<uint8_t> raw(stride * rows);
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols; ++x) {
            const uint8_t* s = data + ((size_t)cols * y + x) * 3;
            uint8_t* d = &raw[stride * y + 1 + (size_t)x * 3];
            d[0] = s[2], d[1] = s[1], d[2] = s[0];
        }
    return write_png_rows(path, raw, rows, cols, 2);
}

}  // namespace o3dr_host
