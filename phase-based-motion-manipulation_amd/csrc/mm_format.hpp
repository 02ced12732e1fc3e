// mm_format.hpp — the one table of frame formats (include/mm.h), host only:
// what the host code needs to know about a format is a field of its row, and a
// new format is a new row plus its kernel instances (DESIGN.md "The format
// table").  Included by mm_impl.hpp after the kernels, whose instance codes
// (kFmt*) the rows name; no kernel reads the table.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/mm.h"

static constexpr int kMatrixBits = MM_MATRIX_BT709 | MM_MATRIX_BT2020;
static constexpr int kRangeBit = 1;   // MM_*_FULL = MM_* | 1 on every Y'CbCr code

static_assert(kFmtNV12 == MM_NV12, "the kernels' NV12 template argument is the format code");
static_assert(kFmtY8 == MM_Y8 && kFmtY16 == MM_Y16, "the kernels' single-plane template arguments are the format codes");
static_assert(kFmtP010 == MM_P010, "the kernels' P010 template argument is the format code");
static_assert(kFmtNV12M == (MM_NV12 | MM_MATRIX_BT709) && kFmtP010M == (MM_P010 | MM_MATRIX_BT709),
              "K1's matrixed template arguments are the BT.709 limited-range codes");
static_assert(kFmtYUY2 == MM_YUY2 && kFmtYUY2M == (MM_YUY2 | MM_MATRIX_BT709),
              "the kernels' packed 4:2:2 template arguments are the YUY2 limited-range codes");
static_assert(kFmtY210 == MM_Y210 && kFmtY210M == (MM_Y210 | MM_MATRIX_BT709),
              "the kernels' 10-bit packed 4:2:2 template arguments are the Y210 limited-range codes");
static_assert(kFmtI420 < 256 && kFmtI420M < 256 && MM_I420 == (MM_NV12 | MM_PLANAR) && !(MM_PLANAR & (kMatrixBits | MM_ORDER_BGR | 255)),
              "the kernels' three-plane template arguments are internal codes below 256 (a code from 256 names a pair)");
static_assert(kFmtI010 < 256 && kFmtI010M < 256 && MM_I010 == (MM_P010 | MM_PLANAR | MM_LOW_BITS) &&
                  !(MM_LOW_BITS & (kMatrixBits | MM_ORDER_BGR | MM_PLANAR | 255)),
              "the kernels' 10-bit three-plane template arguments are internal codes below 256");
static_assert(kFmtV210 < 256 && kFmtV210M < 256 && MM_V210 == (MM_Y210 | MM_PACK_V210) &&
                  !(MM_PACK_V210 & (kMatrixBits | MM_ORDER_BGR | MM_PLANAR | MM_LOW_BITS | 511)),
              "the kernels' v210 template arguments are internal codes below 256; the pack bit is no other bit");
static_assert(kFmtRGB24 == MM_RGB24 && MM_BGR24 == (MM_RGB24 | MM_ORDER_BGR) && !(MM_ORDER_BGR & kMatrixBits),
              "the kernels' packed RGB template argument is the MM_RGB24 code; the order bit is no matrix bit");
static_assert(kFmtBGRA8 < 256 && kFmtBGRA8S < 256 && MM_BGRA8 == (MM_RGBA8 | MM_ORDER_BGRA) &&
                  MM_BGRA8_SRGB == (MM_RGBA8_SRGB | MM_ORDER_BGRA) &&
                  !(MM_ORDER_BGRA & (kMatrixBits | MM_ORDER_BGR | MM_PLANAR | MM_LOW_BITS | MM_PACK_V210 | 511)),
              "the kernels' BGRA template arguments are internal codes below 256; the order bit is no other bit");
static_assert((MM_NV12_FULL ^ MM_NV12) == kRangeBit && (MM_P010_FULL ^ MM_P010) == kRangeBit &&
                  (MM_I420_FULL ^ MM_I420) == kRangeBit && (MM_I010_FULL ^ MM_I010) == kRangeBit &&
                  (MM_YUY2_FULL ^ MM_YUY2) == kRangeBit && (MM_UYVY_FULL ^ MM_UYVY) == kRangeBit &&
                  (MM_Y210_FULL ^ MM_Y210) == kRangeBit && (MM_V210_FULL ^ MM_V210) == kRangeBit,
              "the full-range code of a Y'CbCr format is its limited-range code with bit 0 set");

struct FmtInfo {
    int code;           // the row's public code, with none of the optional bits
    int opt;            // bits a code of this row may carry besides: the range bit and one
                        // matrix bit (Y'CbCr), the byte-order bit (packed RGB)
    int kfmt;           // the kernels' FMT instance (MM_FMT_SWITCH)
    int k1m;            // K1's instance of a code with a matrix bit (MM_FMT_SWITCH_K1; 0: none)
    uint8_t sample;     // bytes of one sample
    uint8_t unit;       // what pitches, offsets, strides and frame pointers are multiples of
    uint8_t bpp;        // bytes per pixel of a row of the first plane
    uint8_t planes;     // 1; 2: a (Cb, Cr) plane; 3: a Cb and a Cr plane, the Cr plane
                        // chroma_pitch x its rows after the Cb plane (mm_surface has one chroma offset)
    uint8_t c_row_div;  // a chroma plane's row bytes: the first plane's over this
    uint8_t c_h_div;    // ... and its rows: H over this
    uint8_t shift;      // 16-bit Y'CbCr words: the code's position (P010, Y210: 6; I010: 0)
    uint8_t order;      // the order uniform (Geo::Lay::yb) of the code without the order bit: UYVY 1
    int max;            // the largest code of a sample (0: float, no code)
    double mean;        // the compose's chroma weight: 0.25, the mean of a 2 x 2 block's four;
                        // 0.5, of a macropixel's two
    // The fused compose's quads (k_rows_inv_compose, k_rows_inv_compose4): what
    // the row starts of {input luma, input chroma, output luma, output chroma}
    // must be multiples of beyond the unit (1: nothing), rows_aligned.  A valid
    // layout that fails takes the unfused pair, whose accesses are single
    // samples: same arithmetic, same results.
    uint8_t quad[4];
    // A grouped format (v210) has no bytes per pixel (bpp 0): grp_px pixels lie
    // in grp_bytes bytes, a partial last group takes the whole dwords its pixels'
    // share of the group needs (2 of 6 pixels: 2 dwords, 4: 3), and the tight
    // frame's pitch is the row's bytes rounded up to tight_align (v210: the 128
    // of every SDK).  0, 0, 0: a row is W x bpp bytes, tight rows back to back.
    // No fused compose reads such a format (k34_fits).
    uint8_t grp_px, grp_bytes, tight_align;

    bool ycc() const { return (opt & kMatrixBits) != 0; }   // Y'CbCr: range and matrix bits, even sizes, no debug view
    bool full(int fmt) const { return ycc() && (fmt & kRangeBit); }
    size_t row_bytes(int W) const
    {
        if (!grp_px) return (size_t)W * bpp;
        const size_t rem = (size_t)(W % grp_px);
        return (size_t)(W / grp_px) * grp_bytes + 4 * ((rem * grp_bytes + 4 * grp_px - 1) / (4 * grp_px));
    }
    // the tight frame's pitch
    size_t tight_pitch(int W) const
    {
        const size_t rb = row_bytes(W);
        return tight_align ? (rb + tight_align - 1) / tight_align * tight_align : rb;
    }
    size_t chroma_row_bytes(int W) const { return row_bytes(W) / c_row_div; }
    size_t frame_bytes(int W, int H) const
    {
        const size_t luma = tight_pitch(W) * (size_t)H;
        return planes == 1 ? luma : luma + (planes - 1) * chroma_row_bytes(W) * (size_t)(H / c_h_div);
    }
};

static constexpr int kYccBits = kRangeBit | kMatrixBits;
static constexpr FmtInfo kFormats[] = {
    // code       opt           kfmt           k1m      smp unit bpp pl cw ch sh ord  max   mean  quad
    // RGBA: quads are multi-dword accesses at dword-aligned addresses, which the
    // unit gives every layout (mm_kernels.hpp ld_quad_a4)
    {MM_RGBA8,      0,          MM_RGBA8,      0,        1,  4,  4, 1, 1, 1, 0, 0,   255, 0.0,  {1, 1, 1, 1}},
    {MM_RGBA32F,    0,          MM_RGBA32F,    0,        4, 16, 16, 1, 1, 1, 0, 0,     0, 0.0,  {1, 1, 1, 1}},
    {MM_RGBA16F,    0,          MM_RGBA16F,    0,        2,  8,  8, 1, 1, 1, 0, 0,     0, 0.0,  {1, 1, 1, 1}},
    {MM_RGBA8_SRGB, 0,          MM_RGBA8_SRGB, 0,        1,  4,  4, 1, 1, 1, 0, 0,   255, 0.0,  {1, 1, 1, 1}},
    // B G R A (MM_ORDER_BGRA on the two 4-byte UNORM codes): MM_RGBA8's fields,
    // instances of their own (the order is compiled in, mm_kernels.hpp PixU8)
    {MM_BGRA8,      0,          kFmtBGRA8,     0,        1,  4,  4, 1, 1, 1, 0, 0,   255, 0.0,  {1, 1, 1, 1}},
    {MM_BGRA8_SRGB, 0,          kFmtBGRA8S,    0,        1,  4,  4, 1, 1, 1, 0, 0,   255, 0.0,  {1, 1, 1, 1}},
    // Single-plane grayscale: the compose reads no input; its quads are stores
    // alone, four bytes as one dword, four words as one 8-byte store at a
    // dword-aligned address.  Units 1 and 2: 98 x 62 MM_Y8 (rows 98 bytes apart) fails.
    {MM_Y8,         0,          kFmtY8,        0,        1,  1,  1, 1, 1, 1, 0, 0,   255, 0.0,  {1, 1, 4, 1}},
    {MM_Y10,        0,          kFmtY16,       0,        2,  2,  2, 1, 1, 1, 0, 0,  1023, 0.0,  {1, 1, 4, 1}},
    {MM_Y12,        0,          kFmtY16,       0,        2,  2,  2, 1, 1, 1, 0, 0,  4095, 0.0,  {1, 1, 4, 1}},
    {MM_Y16,        0,          kFmtY16,       0,        2,  2,  2, 1, 1, 1, 0, 0, 65535, 0.0,  {1, 1, 4, 1}},
    // Packed RGB (MM_BGR24: the order bit): a quad is 12 bytes at 3 X (X % 4 == 0)
    // from the row's start, one dwordx3 load and one dwordx3 store typed 4-byte
    // aligned, on both sides (every tight frame with W % 8 == 0).  Unit 1, a real
    // [H, W, 3] array or a region of one starts at any byte: a region of interest
    // at byte offset 21 or a pitch of 3 W + 3 fails.
    {MM_RGB24,      MM_ORDER_BGR, kFmtRGB24,   0,        1,  1,  3, 1, 1, 1, 0, 0,   255, 0.0,  {4, 1, 4, 1}},
    // NV12: two (Cb, Cr) pairs are read, four luma codes or two pairs stored, as
    // ONE dword at column X % 4 == 0, so every row touched starts on a multiple
    // of 4 (the compose reads no input luma).  Unit 2, so a valid layout may fail.
    // (k_convert also reads a luma dword per row: convert_quads_aligned.)
    {MM_NV12,       kYccBits,   kFmtNV12,      kFmtNV12M, 1, 2,  1, 2, 1, 2, 0, 0,   255, 0.25, {1, 4, 4, 4}},
    // P010: 8-byte luma and 4-byte chroma accesses at dword-aligned addresses, its unit
    {MM_P010,       kYccBits,   kFmtP010,      kFmtP010M, 2, 4,  2, 2, 1, 2, 6, 0,  1023, 0.25, {1, 1, 1, 1}},
    // Three-plane 8-bit 4:2:0 (MM_NV12 | MM_PLANAR): four luma codes as one dword
    // store, the quad's two Cb and its two Cr samples as one 2-byte access per
    // plane, loads and stores alike (every tight frame with W % 8 == 0).  Unit 1,
    // chroma rows of W / 2 bytes start at any byte: 98 x 62 (chroma rows of 49 bytes) fails.
    {MM_I420,       kYccBits,   kFmtI420,      kFmtI420M, 1, 1,  1, 3, 2, 2, 0, 0,   255, 0.25, {1, 2, 4, 2}},
    // Its 10-bit form (MM_P010 | MM_PLANAR | MM_LOW_BITS), codes in the words' low
    // bits: four luma codes as one 8-byte store at a dword-aligned address, two
    // Cb words and two Cr words as one dword per plane.  Unit 2, one word: a base,
    // a pitch or a plane offset at 2 mod 4 fails.  These numbers speak of row
    // STARTS alone: that a quad's dword of two chroma words ends inside its row is
    // k34_fits' own W % 8 == 0, which refuses a frame such as 98 x 62 whatever
    // they say (do not lift that condition on the strength of them).
    {MM_I010,       kYccBits,   kFmtI010,      kFmtI010M, 2, 2,  2, 3, 2, 2, 0, 0,  1023, 0.25, {1, 4, 4, 4}},
    // Packed 4:2:2, one plane of macropixels: 8-bit, four bytes Y0 Cb Y1 Cr
    // (YUY2) or Cb Y0 Cr Y1 (UYVY), quads of 8 bytes at dword-aligned addresses;
    // 10-bit, eight bytes of P010's words Y0 Cb Y1 Cr, quads of 16 bytes at
    // 8-byte-aligned addresses (ld_quad_a8).  The unit, one macropixel, gives both.
    {MM_YUY2,       kYccBits,   kFmtYUY2,      kFmtYUY2M, 1, 4,  2, 1, 1, 1, 0, 0,   255, 0.5,  {1, 1, 1, 1}},
    {MM_UYVY,       kYccBits,   kFmtYUY2,      kFmtYUY2M, 1, 4,  2, 1, 1, 1, 0, 1,   255, 0.5,  {1, 1, 1, 1}},
    {MM_Y210,       kYccBits,   kFmtY210,      kFmtY210M, 2, 8,  4, 1, 1, 1, 6, 0,  1023, 0.5,  {1, 1, 1, 1}},
    // v210 (MM_Y210 | MM_PACK_V210): Y210's samples, six pixels to a group of four
    // dwords, the unit; the kernels read a code as Y210's word code << 6 (shift 6:
    // Y210's uniforms).  Rows of 4 D(W) bytes in a pitch of 128 ceil(W / 48).
    {MM_V210,       kYccBits,   kFmtV210,      kFmtV210M, 4, 16, 0, 1, 1, 1, 6, 0,  1023, 0.5,  {1, 1, 1, 1}, 6, 16, 128},
};

// The row of a format code, or null for a code that is no format: a code is
// its row's code plus any of the row's optional bits, but not both matrix bits.
// (A negative code, a matrix bit on an RGBA or single-plane code, the plane bit
// on anything but NV12 and P010: no row.)
static inline const FmtInfo *fmt_info(int fmt)
{
    for (const FmtInfo &f : kFormats) {
        const int extra = fmt ^ f.code;
        if (!(extra & ~f.opt) && (extra & kMatrixBits) != kMatrixBits) return &f;
    }
    return nullptr;
}
static inline int fmt_matrix(int fmt) { return fmt & kMatrixBits; }

// The code range of a Y'CbCr format: the luma and chroma scales, the luma
// offset (8-bit limited: Y 16 .. 235, C 16 .. 240; 10-bit limited: Y 64 .. 940,
// C 64 .. 960; full: 0 .. max) and the word unit per code (P010, Y210: 64).
struct CodeRange { double ys, cs, y0, u; };
static inline CodeRange code_range(const FmtInfo &f, bool full)
{
    const bool p10 = f.max == 1023;
    return {p10 ? (full ? 1023.0 : 876.0) : (full ? 255.0 : 219.0),
            p10 ? (full ? 1023.0 : 896.0) : (full ? 255.0 : 224.0),
            full ? 0.0 : p10 ? 64.0 : 16.0, (double)(1 << f.shift)};
}

// The planes of one W x H frame in layout s, in memory order: luma (or the one
// plane), then the chroma plane or planes.
struct Plane { size_t offset, pitch, row_bytes, rows; };
// Returns the plane count, 0 where the Cr plane's offset overflows.  (s.format valid.)
static inline int surf_planes(int W, int H, const mm_surface &s, Plane out[3])
{
    const FmtInfo &f = *fmt_info(s.format);
    out[0] = {0, s.pitch, f.row_bytes(W), (size_t)H};
    for (int k = 1; k < f.planes; ++k) {
        out[k] = {s.chroma_offset, s.chroma_pitch, f.chroma_row_bytes(W), (size_t)(H / f.c_h_div)};
        size_t d;
        if (k == 2 && (__builtin_mul_overflow(s.chroma_pitch, out[k].rows, &d) ||
                       __builtin_add_overflow(d, s.chroma_offset, &out[k].offset)))
            return 0;
    }
    return f.planes;
}
