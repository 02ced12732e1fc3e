// mm_kernels.hpp — the three HIP kernels of one magnified frame (gfx950).
//
// Data flow per frame (N = padded square size, F = N/2+1 half-spectrum columns):
//   K1 k_rows_fwd : RGBA frame --(luma, stretch+pad bilinear, Hann window)-->
//                   real rows --(paired real FFT)--> G[f][row]       (f < F)
//   K2 k_cols     : G column --FFT--> F_t --(pyramid phase op vs F_{t-1})-->
//                   A --IFFT--> Q[row/2][f][row%2]; F_t becomes the state.
//                   One FFT group owns a column for a whole chunk of frames, so
//                   F_{t-1} stays in registers between frames.
//   K3 k_rows_inv : Q rows --(paired C2R IFFT)--> |z| --(5-tap H blur)--> Yh
//   K4 k_compose  : Yh --(5-tap V blur)--, input --(I/Q resample)--> YIQ->RGB,
//                   saturate, crop --> RGBA frame
// Reference stages replaced (MotionMagnificationProcessor.cs:145-206): a4-a18 of
// SURVEY.md §8(a).  The pyramid levels are applied pointwise in frequency
// (SURVEY.md §7): arg(m_i F) = arg F for real m_i >= 0, so one atan2/sincos per
// bin serves every level.
#pragma once
#include "mm_fft.hpp"
#include "mm_srgb.hpp"
#include <stdint.h>
#include <type_traits>

namespace mm {

constexpr int kMaxLevels = 16;
constexpr float kPi = 3.14159265359f;  // PyramidOperations.compute:5

struct Tap4 {         // composite stretch+pad bilinear taps incl. Hann factor
    int idx[4];
    float w[4];
};

struct Geo {
    int W, H, N;
    int x0, y0;       // image placement inside the canvas (PadTexture .cs:360-363):
                      // floor((N - W) / 2); for odd N - W the quad's left edge is at
                      // x0 + 0.5 and CropTexture samples between two texels
    int ox, oy;       // W, H odd (k_compose_odd)
    int Hg;           // rows per G column (H rounded up to even: K1 writes row pairs)
    int Wy;           // Yh columns (W + ox: the crop's second texel)
    int rb;           // canvas row of Q list index 0 (= y0 - 2)
    int Hn;           // rows kept in Q (= min(H + 4, N))
    int Hq;           // Hn rounded up to whole Q tiles (TK rows)
    int Qs;           // Q bins per tile row (N/2 + 2; q_index)
    int TK;           // rows per Q tile (q_tile_v)
    int edge;         // 0 repeat, 1 clamp
    // MM_NV12 / MM_NV12_FULL only (the two ranges share the kernel instances;
    // filled per launch by geo_of, mm_impl.hpp; the other formats never read it).
    // MM_P010 / MM_P010_FULL use it the same way, in units of the 16-bit word
    // on input (64 per 10-bit code: y_off 64 x, y_unit and the matrix 1/64 x)
    // and of the 10-bit code on output (chroma bias 512.5, not 128.5).
    // A matrix bit (MM_MATRIX_BT709 / _BT2020) changes values only, except in
    // K1, whose matrixed instances add the chroma term of RGBToYIQ's luma.
    struct Nv12 {
        float y_off, y_unit;        // K1: luma = ((float)Yb - y_off) * y_unit
        float la, lb;               // K1, matrixed: ... + la (Cb - mid) + lb (Cr - mid) inside the bracket:
                                    // Yq's a, b times luma / chroma code scale (BT.601: 0, never read)
        float icb, qcb, icr, qcr;   // compose: (I, Q) = (icb, qcb) (Cb - 128) + (icr, qcr) (Cr - 128),
                                    // RGBToYIQ x BT.601 with the code scale folded in
        float kr, kg, kb;           // out: Yl = kr R + kg G + kb B, the matrix's luma weights
        float yo_scale, yo_bias;    // out: luma code = floor(Yl * yo_scale + yo_bias), bias = offset + 0.5
        float cbo, cro;             // out: chroma code = floor(sum of four (B - Yl) * cbo + 128.5), Cr: R - Yl
                                    // (packed 4:2:2: the sum of the macropixel's two)
    } nv;
    // Where the caller's frames lie (mm_surface, include/mm.h), in bytes, the
    // input side (li) and the output side (lo) apart; filled per launch by
    // geo_of.  Row r of the RGBA / luma plane at r * pitch, (Cb, Cr) row j at
    // c_off + j * c_pitch, frame k at k * stride.  Every offset inside a frame
    // fits 32 bits (extent <= 2^32, mm_surface_bytes): workgroup-uniform row
    // bases plus 32-bit lane offsets, as with the tight layout's W * bpp.
    // yb (packed 4:2:2 only, else 0): the side's byte order, Y0's byte in the
    // macropixel (YUY2 0, UYVY 1); Cb's is 1 - yb, Y1 and Cr lie two bytes on.
    struct Lay {
        unsigned pitch, c_off, c_pitch, yb;
        size_t stride;
    } li, lo;
};

struct Spec {
    int mode;               // MM_MODE_PYRAMID (0) | MM_MODE_STANDARD (1)
    // standard mode band-pass (PhaseDifferenceComputeShader.compute:88-122)
    int bp_apply;
    float bp_low, bp_high, bp_steep, bp_sens, bp_edge;
    float bp_inv_low, bp_inv_1mhigh, bp_inv_band;
    int L;
    float minF, maxF, S, tau2, inv_nn;
    float S_rev;            // S / (2 pi): phase scale in revolutions (v_sin/v_cos)
    float tau2_nn;          // tau2 * inv_nn^2 (gate on masks pre-scaled by inv_nn)
    float hp_lo, hp_inv;    // high-pass ramp start maxF*0.8, 1/(maxF*0.2)
    float lp_hi, lp_inv;    // low-pass ramp end minF*1.2, 1/(minF*0.2)
    float lo[kMaxLevels], hi[kMaxLevels], inv_w[kMaxLevels];  // middle bands
    // MM_MODE_STEERABLE (mm_steer.hpp): orientations, filter, IIR coefficients,
    // orientation unit vectors (cos, sin of 2 pi k / O)
    int O, filt;
    float r_low, r_high;
    float ang_c[8], ang_s[8];
};

struct Blur5 {
    float w0, w1, w2;   // taps at 0, +-1, +-2 texels
    float c0, c1, c2;   // 255 x the taps, each product rounded once from double (build_blur):
                        // the RGBA8 compose's vertical blur, in code units (yiq_rgba8)
};

constexpr int ilog2c(int x) { return x <= 1 ? 0 : 1 + ilog2c(x / 2); }
template <int LOG2N> constexpr int fft_T() { return (1 << LOG2N) / 8; }
template <int LOG2N> constexpr int groups_per_wg() { return fft_T<LOG2N>() >= 256 ? 1 : 256 / fft_T<LOG2N>(); }
template <int LOG2N> constexpr int wg_threads() { return groups_per_wg<LOG2N>() * fft_T<LOG2N>(); }
// at least MIN FFT groups per workgroup (within 1024 threads)
constexpr int groups_at_least_v(int log2n, int min)
{
    const int T = (1 << log2n) / 8, base = T >= 256 ? 1 : 256 / T;
    if (base >= min) return base;
    int g = min;
    while (g > base && T * g > 1024) g /= 2;
    return g;
}
template <int LOG2N, int MIN> constexpr int groups_at_least() { return groups_at_least_v(LOG2N, MIN); }
#ifndef MM_K1_GROUPS
#define MM_K1_GROUPS 2
#endif
#ifndef MM_K2_GROUPS
#define MM_K2_GROUPS 2
#endif
#ifndef MM_K3_GROUPS
#define MM_K3_GROUPS 1
#endif
// K3 runs one Q tile (TK = 2 * groups rows) per workgroup
template <int LOG2N> constexpr int k3_groups() { return groups_at_least<LOG2N, MM_K3_GROUPS>(); }
template <int LOG2N> constexpr int k3_threads() { return k3_groups<LOG2N>() * fft_T<LOG2N>(); }
// (MM_Q_TILE_8K: rows per Q tile at N = 8192, where K3 runs one row pair per
// workgroup: 4 gives K2 32-B Q pieces from its one column per workgroup.
// 5120x2880 same-call, tiles of 2 / 4 / 8 rows: K2 193-196 / 185 / 179-184 us,
// K3 31 / 35 / 45 us per frame, 3.04-3.11k / 3.13k / 3.04-3.10k frames/s,
// profiles/r06k_q_tile_8k_ab.txt)
#ifndef MM_Q_TILE_8K
#define MM_Q_TILE_8K 4
#endif
constexpr int q_tile_v(int log2n) { return log2n == 13 ? MM_Q_TILE_8K : 2 * groups_at_least_v(log2n, MM_K3_GROUPS); }
template <int LOG2N> constexpr int q_tile() { return q_tile_v(LOG2N); }
// K1 runs >= 2 row pairs per workgroup so that G receives 32-B pieces
template <int LOG2N> constexpr int k1_groups() { return groups_at_least<LOG2N, MM_K1_GROUPS>(); }
template <int LOG2N> constexpr int k1_threads() { return k1_groups<LOG2N>() * fft_T<LOG2N>(); }
// LAT: short launches (one frame: the drop-in call) run one row pair per
// workgroup, so that twice as many workgroups spread over the CUs and none
// waits behind another's latency chain (G then leaves as 16-B pieces)
template <int LOG2N, bool LAT> constexpr int k1_gpw() { return LAT && fft_T<LOG2N>() >= 64 ? 1 : k1_groups<LOG2N>(); }

__device__ __forceinline__ int wrap_idx(int i, int n, int edge)
{
    if (edge) return i < 0 ? 0 : (i >= n ? n - 1 : i);
    int r = i % n;
    return r < 0 ? r + n : r;
}

// Wrap an index known to lie in [-1, n] (resample taps) with the edge mode.
__device__ __forceinline__ int wrap_near(int i, int n, int edge)
{
    if (i < 0) return edge ? 0 : i + n;
    if (i >= n) return edge ? n - 1 : i - n;
    return i;
}

// Same-XCD blocks (b % 8 equal under round-robin dispatch) get consecutive ids.
__device__ __forceinline__ int xcd_remap(int b, int nb)
{
    int q = nb / 8, r = nb % 8, x = b % 8;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + b / 8;
}

// Like xcd_remap, but each XCD owns runs of G consecutive blocks spread over the
// whole range (run k on XCD k % 8): same-XCD neighbours still share L2 lines,
// and work that varies smoothly with the block index is balanced over XCDs.
// Falls back to xcd_remap when nb is not a multiple of 8 G.
template <int G>
__device__ __forceinline__ int xcd_interleave(int b, int nb)
{
    if (nb % (8 * G) != 0) return xcd_remap(b, nb);
    const int x = b % 8, q = b / 8;
    return ((q / G) * 8 + x) * G + q % G;
}

// Access at a 32-bit BYTE offset from a (workgroup-uniform) base: matches the
// scalar-base + 32-bit vector-offset form of global loads/stores (an index
// scaled as zext(i) * sizeof(T) needs 64-bit address math per access).
template <class T>
__device__ __forceinline__ T ld_off(const void *base, unsigned byte_off)
{
    return *reinterpret_cast<const T *>(reinterpret_cast<const uint8_t *>(base) + byte_off);
}
template <class T>
__device__ __forceinline__ void st_off(void *base, unsigned byte_off, T v)
{
    *reinterpret_cast<T *>(reinterpret_cast<uint8_t *>(base) + byte_off) = v;
}

// Stores of whole 128-B lines that nothing reads back soon (output frames, Yh
// rows): non-temporal, so that they stream out under the kernel instead of
// sitting dirty in L2 for the write-back at the end of the kernel (same-call:
// K34 -4 %, one-frame K3 / K4 -5 % / -7 %).  The partial-line hand-off stores
// (G, Q) stay write-back: their pieces are merged in L2 (non-temporal there:
// K1 3x, K2 1.8x slower, profiles/r03g_nt_ab.txt).
template <class T>
__device__ __forceinline__ void st_stream(void *base, unsigned byte_off, T v)
{
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    void *p = reinterpret_cast<uint8_t *>(base) + byte_off;
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    if constexpr (sizeof(T) == 16) {
        u32x4 w;
        __builtin_memcpy(&w, &v, 16);
        __builtin_nontemporal_store(w, reinterpret_cast<u32x4 *>(p));
    } else if constexpr (sizeof(T) == 8) {
        u32x2 w;
        __builtin_memcpy(&w, &v, 8);
        __builtin_nontemporal_store(w, reinterpret_cast<u32x2 *>(p));
    } else {
        static_assert(sizeof(T) == 4, "st_stream: 4, 8 or 16 bytes");
        unsigned w;
        __builtin_memcpy(&w, &v, 4);
        __builtin_nontemporal_store(w, reinterpret_cast<unsigned *>(p));
    }
}

// The fused kernels' RGBA8 quads (16 bytes) and P010 quads (four words, 8
// bytes) at a dword-aligned address.  A surface's rows start on multiples of
// its unit, 4 bytes, and not always on multiples of 16 or 8 (a pitch of row
// bytes + 4, a region of interest at an odd column, a stream whose frames are
// 4 mod 8 apart); gfx9 global memory takes a multi-dword access at any
// dword-aligned address, so the quad stays one access in every layout, typed
// with the alignment it really has.
typedef unsigned u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ uint4 ld_quad_a4(const void *base, unsigned byte_off)
{
    const u32x4_a4 w = *reinterpret_cast<const u32x4_a4 *>(reinterpret_cast<const uint8_t *>(base) + byte_off);
    return make_uint4(w.x, w.y, w.z, w.w);
}
__device__ __forceinline__ void st_stream_quad_a4(void *base, unsigned byte_off, uint4 v)
{
    u32x4_a4 w;
    __builtin_memcpy(&w, &v, 16);
    __builtin_nontemporal_store(w, reinterpret_cast<u32x4_a4 *>(reinterpret_cast<uint8_t *>(base) + byte_off));
}

// ... and MM_Y210 quads (two 8-byte macropixels) at an 8-byte-aligned address
typedef unsigned u32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));
__device__ __forceinline__ uint4 ld_quad_a8(const void *base, unsigned byte_off)
{
    const u32x4_a8 w = *reinterpret_cast<const u32x4_a8 *>(reinterpret_cast<const uint8_t *>(base) + byte_off);
    return make_uint4(w.x, w.y, w.z, w.w);
}
__device__ __forceinline__ void st_stream_quad_a8(void *base, unsigned byte_off, uint4 v)
{
    u32x4_a8 w;
    __builtin_memcpy(&w, &v, 16);
    __builtin_nontemporal_store(w, reinterpret_cast<u32x4_a8 *>(reinterpret_cast<uint8_t *>(base) + byte_off));
}

typedef unsigned u32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));
__device__ __forceinline__ void st_stream_pair_a4(void *base, unsigned byte_off, unsigned lo, unsigned hi)
{
    u32x2_a4 w;
    w.x = lo;
    w.y = hi;
    __builtin_nontemporal_store(w, reinterpret_cast<u32x2_a4 *>(reinterpret_cast<uint8_t *>(base) + byte_off));
}
__device__ __forceinline__ uint2 ld_pair_a4(const void *base, unsigned byte_off)
{
    const u32x2_a4 w = *reinterpret_cast<const u32x2_a4 *>(reinterpret_cast<const uint8_t *>(base) + byte_off);
    return make_uint2(w.x, w.y);
}

// |z| rows of the row IFFTs (K3 four-wide path, K34, K34o) start kZShift
// floats into their LDS row, so that the blur taps c-2 .. c+5 of an aligned
// quad c = x0 + 4q (x0 % 4 == 0) are two 16-B aligned ds_read_b128.
constexpr int kZShift = 2;

// Q hand-off (K2 -> K3): element (row k, bin f) of a frame, stored in tiles of
// TK rows: [k/TK][f][k%TK], Qs bins per tile row.  A K2 workgroup's columns of
// one tile are contiguous (GPW*TK*8 bytes: whole 128-B lines at TK = 8), and
// K3's TK/2 row pairs of a bin are one contiguous TK*8-byte block.
__device__ __forceinline__ size_t q_index(const Geo &g, int k, int f)
{
    return ((size_t)(k / g.TK) * g.Qs + f) * g.TK + (k % g.TK);
}

#ifdef MM_ASM_MARKS
#define MM_MARK(x) asm volatile("; " x)
#else
#define MM_MARK(x)
#endif

// ---- pixel access -------------------------------------------------------
template <int FMT> struct Pix;
// The 4-byte UNORM pixel in either byte order: R G B A (ORD 0: MM_RGBA8) or
// B G R A (ORD 1: MM_BGRA8 = MM_RGBA8 | MM_ORDER_BGRA).  A BGRA frame IS the
// RGBA8 frame with bytes 0 and 2 of every pixel exchanged (include/mm.h), and
// the exchange is made at compile time: the order names which byte each
// convert, shift and dot weight touches, never how many instructions there are,
// and every value computed from (r, g, b) is the other order's bit for bit.
// The public codes carry MM_ORDER_BGRA (8192), so the instances are internal
// codes below 256 (0 | 128, 3 | 128), as the three-plane formats' are.
constexpr int kFmtBGRA8 = 128;    // MM_BGRA8
constexpr int kFmtBGRA8S = 131;   // MM_BGRA8_SRGB
template <int FMT> constexpr bool kBGRA = FMT == kFmtBGRA8 || FMT == kFmtBGRA8S;
template <int FMT> constexpr bool kRGBA8u = FMT == 0 || FMT == kFmtBGRA8;   // linear UNORM bytes, either order
template <int ORD> struct PixU8 {     // RGBA8 / BGRA8 UNORM
    static constexpr int bpp = 4;
    static constexpr unsigned rb = ORD ? 2u : 0u, bb = ORD ? 0u : 2u;   // the bytes of R and B (G: 1, A: 3)
    static constexpr unsigned rs = 8u * rb, bs = 8u * bb;
    using raw_t = uint32_t;             // keep loads raw in registers, convert at use
    __device__ static raw_t raw(const uint8_t *base, size_t i)
    {
        return reinterpret_cast<const uint32_t *>(base)[i];
    }
    __device__ static float4 cvt(raw_t u)
    {
        const float s = 1.0f / 255.0f;
        return make_float4((float)((u >> rs) & 255u) * s, (float)((u >> 8) & 255u) * s,
                           (float)((u >> bs) & 255u) * s, (float)(u >> 24) * s);
    }
    __device__ static float4 load(const uint8_t *base, size_t i) { return cvt(raw(base, i)); }
    __device__ static uint32_t pack(float r, float g, float b)
    {
        uint32_t R = (uint32_t)(r * 255.0f + 0.5f), G = (uint32_t)(g * 255.0f + 0.5f),
                 B = (uint32_t)(b * 255.0f + 0.5f);
        return (R << rs) | (G << 8) | (B << bs) | (255u << 24);
    }
    __device__ static void store(uint8_t *base, unsigned i, float r, float g, float b)
    {
        st_stream<uint32_t>(base, i * 4u, pack(r, g, b));
    }
    // r, g, b in code units (255 x the UNORM value), neither saturated nor
    // rounded: three v_cvt_pk_u8_f32, each clamping to 0 .. 255 and rounding to
    // nearest even into its byte lane (tools/cvtpk_probe.hip), alpha 255.
    // (0xff000000 is no inline constant: left to the compiler it sits in a
    // VGPR for the whole kernel, which at the fused compose's 128-VGPR bound
    // is a spill; made opaque in a scalar register it stays there.)
    __device__ static uint32_t pack_codes(float r, float g, float b)
    {
        uint32_t alpha = 0xff000000u;
        asm("" : "+s"(alpha));
        const uint32_t a = __builtin_amdgcn_cvt_pk_u8_f32(r, rb, alpha);
        return __builtin_amdgcn_cvt_pk_u8_f32(b, bb, __builtin_amdgcn_cvt_pk_u8_f32(g, 1u, a));
    }
};
template <> struct Pix<0> : PixU8<0> {};
template <> struct Pix<kFmtBGRA8> : PixU8<1> {};
template <> struct Pix<1> {           // RGBA32F
    static constexpr int bpp = 16;
    using raw_t = float4;
    __device__ static raw_t raw(const uint8_t *base, size_t i)
    {
        return reinterpret_cast<const float4 *>(base)[i];
    }
    __device__ static float4 cvt(raw_t v) { return v; }
    __device__ static float4 load(const uint8_t *base, size_t i) { return raw(base, i); }
    __device__ static void store(uint8_t *base, unsigned i, float r, float g, float b)
    {
        st_stream<float4>(base, i * 16u, make_float4(r, g, b, 1.0f));
    }
};
// RGBA16F: linear half floats, as the reference camera's HDR render target
// (ARGBHalf: Assets/Scenes/SampleScene.unity:663 m_HDR, linear colour space
// ProjectSettings/ProjectSettings.asset:50) hands them to OnRenderImage
// (.cs:101).  Values above 1 pass unclipped up to the reference's saturate
// (YIQToRGB.shader); the output is rounded to half (round to nearest even).
template <> struct Pix<2> {
    static constexpr int bpp = 8;
    using raw_t = uint2;
    __device__ static raw_t raw(const uint8_t *base, size_t i)
    {
        return reinterpret_cast<const uint2 *>(base)[i];
    }
    __device__ static float h2f(unsigned bits)
    {
        return (float)__builtin_bit_cast(_Float16, (unsigned short)(bits & 0xffffu));
    }
    __device__ static unsigned f2h(float v)
    {
        return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)v);
    }
    __device__ static float4 cvt(raw_t u)
    {
        return make_float4(h2f(u.x), h2f(u.x >> 16), h2f(u.y), h2f(u.y >> 16));
    }
    __device__ static uint2 pack(float r, float g, float b)
    {
        return make_uint2(f2h(r) | f2h(g) << 16, f2h(b) | 0x3C00u << 16);   // alpha 1.0
    }
    __device__ static void store(uint8_t *base, unsigned i, float r, float g, float b)
    {
        st_stream<uint2>(base, i * 8u, pack(r, g, b));
    }
};
// RGBA8 sRGB: an 8-bit sRGB render target under Unity's Linear colour space
// is sampled as linear light and encoded on write, so the pipeline sees
// linear values.  Decode: the exact 256-entry table (tools/gen_srgb.py);
// encode of a saturated value: 255 srgb(v) rounded, found from the pow
// approximation and corrected by one step against the exact thresholds
// kSrgbThr (the approximation is within one code of the exact one).
template <int ORD> struct PixS8 {     // ORD as PixU8's: 0 R G B A, 1 B G R A (MM_BGRA8_SRGB)
    static constexpr int bpp = 4;
    static constexpr unsigned rs = PixU8<ORD>::rs, bs = PixU8<ORD>::bs;
    using raw_t = uint32_t;
    __device__ static raw_t raw(const uint8_t *base, size_t i)
    {
        return reinterpret_cast<const uint32_t *>(base)[i];
    }
    __device__ static float4 cvt(raw_t u)
    {
        return make_float4(kSrgbDec[(u >> rs) & 255u], kSrgbDec[(u >> 8) & 255u], kSrgbDec[(u >> bs) & 255u],
                           (float)(u >> 24) * (1.0f / 255.0f));
    }
    __device__ static uint32_t enc(float v)
    {
        const float s = v <= 0.0031308f ? 12.92f * v : 1.055f * __powf(v, 1.0f / 2.4f) - 0.055f;
        int b = min(max((int)(s * 255.0f + 0.5f), 0), 255);
        b += v >= kSrgbThr[b + 1] ? 1 : 0;
        b -= v < kSrgbThr[b] ? 1 : 0;
        return (uint32_t)b;
    }
    __device__ static uint32_t pack(float r, float g, float b)
    {
        return (enc(r) << rs) | (enc(g) << 8) | (enc(b) << bs) | (255u << 24);
    }
    __device__ static void store(uint8_t *base, unsigned i, float r, float g, float b)
    {
        st_stream<uint32_t>(base, i * 4u, pack(r, g, b));
    }
};
template <> struct Pix<3> : PixS8<0> {};
template <> struct Pix<kFmtBGRA8S> : PixS8<1> {};
// saturated before the store: the UNORM destinations (RGBA8, RGBA8 sRGB, in either byte order)
template <int FMT> constexpr bool kUnorm = FMT == 0 || FMT == 3 || kBGRA<FMT>;

// RGBToYIQ.shader:46-50 rows
__device__ __forceinline__ float luma(float4 c) { return 0.299f * c.x + 0.587f * c.y + 0.114f * c.z; }
__device__ __forceinline__ float chroma_i(float4 c) { return 0.596f * c.x + -0.274f * c.y + -0.322f * c.z; }
__device__ __forceinline__ float chroma_q(float4 c) { return 0.211f * c.x + -0.523f * c.y + 0.312f * c.z; }
__device__ __forceinline__ float sat(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// Y of a raw pixel (RGBA8: 1/255 folded into the RGBToYIQ row).
// K1's luma in units of kLumaUnit<FMT>: RGBA8 as the exact integer
// 299 R + 587 G + 114 B (two v_dot4_u32_u8: 299 = 256 + 43, 587 = 2 * 256 + 75,
// and one convert; RGBToYIQ's 0.299/0.587/0.114 of R/255 ... times 255000),
// whose unit 1/255000 folds into the resample weights; RGBA32F as luma().
template <int FMT> constexpr float kLumaUnit = kRGBA8u<FMT> ? 1.0f / 255000.0f : 1.0f;
template <int FMT>
__device__ __forceinline__ float luma_units(typename Pix<FMT>::raw_t u)
{
    if constexpr (kRGBA8u<FMT>) {   // (B G R A: the weights on the other bytes, rgb24_luma_units' for that order)
        constexpr unsigned w_hi = 2u << 8 | 1u << Pix<FMT>::rs;
        constexpr unsigned w_lo = 43u << Pix<FMT>::rs | 75u << 8 | 114u << Pix<FMT>::bs;
        static_assert(FMT != 0 || (w_hi == 0x00000201u && w_lo == 0x00724B2Bu), "MM_RGBA8's weights");
        static_assert(FMT == 0 || (w_hi == 0x00010200u && w_lo == 0x002B4B72u), "MM_BGRA8's weights");
        const unsigned hi = __builtin_amdgcn_udot4(u, w_hi, 0u, false);    // R + 2 G
        return (float)__builtin_amdgcn_udot4(u, w_lo, hi << 8, false);   // + 43 R + 75 G + 114 B
    } else {
        return luma(Pix<FMT>::cvt(u));
    }
}

// (I, Q) of a raw pixel.  RGBA8: the 1/255 of the UNORM read is folded into the
// RGBToYIQ coefficients (3 byte converts + 6 FMAs).
template <int FMT>
__device__ __forceinline__ float2 chroma_iq(typename Pix<FMT>::raw_t u)
{
    if constexpr (kRGBA8u<FMT>) {
        constexpr float k = 1.0f / 255.0f;
        const float r = (float)((u >> Pix<FMT>::rs) & 255u), gg = (float)((u >> 8) & 255u),
                    b = (float)((u >> Pix<FMT>::bs) & 255u);
        return make_float2((0.596f * k) * r + (-0.274f * k) * gg + (-0.322f * k) * b,
                           (0.211f * k) * r + (-0.523f * k) * gg + (0.312f * k) * b);
    } else {
        const float4 c = Pix<FMT>::cvt(u);
        return make_float2(chroma_i(c), chroma_q(c));
    }
}

// Packed-FP32 pixel math of the compose stage (K4 and K34 share it, so the
// fused and unfused outputs stay bitwise equal): (I, Q) is one c2, and every
// weighted sum is written in the same left-to-right order as its scalar form,
// so each lane computes the scalar form's fma chain exactly (v_pk_fma_f32 /
// v_pk_mul_f32 with a broadcast scalar operand: half the VALU instructions).
template <int FMT>
__device__ __forceinline__ c2 chroma_iq2(typename Pix<FMT>::raw_t u)
{
    if constexpr (kRGBA8u<FMT>) {
        constexpr float k = 1.0f / 255.0f;
        const float r = (float)((u >> Pix<FMT>::rs) & 255u), gg = (float)((u >> 8) & 255u),
                    b = (float)((u >> Pix<FMT>::bs) & 255u);
        return mk(0.596f * k, 0.211f * k) * r + mk(-0.274f * k, -0.523f * k) * gg + mk(-0.322f * k, 0.312f * k) * b;
    } else {
        const float4 c = Pix<FMT>::cvt(u);
        return mk(0.596f, 0.211f) * c.x + mk(-0.274f, -0.523f) * c.y + mk(-0.322f, 0.312f) * c.z;
    }
}

// YIQToRGB.shader:51-76 + saturate for one pixel: R and G as one pair, B alone
// (B as two FMAs: written as 1 yb + ..., the contraction fused the 1 yb
// product and left a multiply and a subtract)
__device__ __forceinline__ void yiq_rgb(float yb, c2 cc, float &rr, float &gg, float &bb)
{
    const c2 rg = mk(yb, yb) + mk(0.956f, -0.272f) * cc.x + mk(0.621f, -0.647f) * cc.y;
    const float b = fmaf(1.703f, cc.y, fmaf(-1.106f, cc.x, yb));
    rr = sat(rg.x); gg = sat(rg.y); bb = sat(b);
}
// RGBA8 UNORM out: the same pixel straight to its four bytes, in code units.
// yc is 255 x Y' (the vertical blur with Blur5::c0 .. c2), the matrix carries
// the 255 for (I, Q) (each product rounded once, the same in every instance),
// and YIQToRGB's saturate and the UNORM write's x 255 + round are the clamp and
// round-to-nearest-even of the packed byte convert (Pix<0>::pack_codes): 3 VALU
// per pixel behind the matrix instead of 3 saturates, 3 FMAs, 3 converts and
// the byte merge.  Every compose kernel that writes RGBA8 calls this one
// definition (k_compose, k_rows_inv_compose, k_rows_inv_compose4), so the
// fused, one-shot and unfused outputs stay bitwise equal.  Against yiq_rgb +
// Pix<0>::pack a byte differs by at most one code, only where the code-unit
// value lies within rounding of a half (or is an exact half: even, not up).
// (sRGB's encode is not linear in the code: MM_RGBA8_SRGB keeps yiq_rgb.)
// Packed RGB out (MM_RGB24 / MM_BGR24: "MM_RGBA8's rule, three bytes",
// include/mm.h) stores three bytes of the same word and stays the RGBA8 path
// byte for byte (tests/test_rgb24.py).
template <int FO> constexpr bool kCodeOut = FO == 0 || FO == 13 || FO == kFmtBGRA8;   // MM_RGBA8, kFmtRGB24 (below), MM_BGRA8
constexpr float kCodeRI = (float)(255.0 * 0.956), kCodeGI = (float)(255.0 * -0.272);
constexpr float kCodeRQ = (float)(255.0 * 0.621), kCodeGQ = (float)(255.0 * -0.647);
constexpr float kCodeBI = (float)(255.0 * -1.106), kCodeBQ = (float)(255.0 * 1.703);
// (FO: the byte order of the word; packed RGB takes RGBA8's and picks its three bytes)
template <int FO = 0> __device__ __forceinline__ uint32_t yiq_rgba8(float yc, c2 cc)
{
    const c2 rg = mk(yc, yc) + mk(kCodeRI, kCodeGI) * cc.x + mk(kCodeRQ, kCodeGQ) * cc.y;
    const float b = fmaf(kCodeBQ, cc.y, fmaf(kCodeBI, cc.x, yc));
    return Pix<FO == kFmtBGRA8 ? kFmtBGRA8 : 0>::pack_codes(rg.x, rg.y, b);
}
// the compose kernels' vertical blur taps for output format FO
struct VBlur { float w0, w1, w2; };
template <int FO> __device__ __forceinline__ VBlur vblur_w(const Blur5 &b)
{
    if constexpr (kCodeOut<FO>) return VBlur{b.c0, b.c1, b.c2};
    else return VBlur{b.w0, b.w1, b.w2};
}

// ---- NV12 (planar 4:2:0) access ------------------------------------------
// A frame is H rows of W luma bytes, then H/2 rows of W bytes of interleaved
// (Cb, Cr) pairs, one pair per 2x2 pixels; W and H even.  It IS the RGBA32F
// frame its BT.601 decode gives (include/mm.h), and the RGBToYIQ rows sum to
// 1, 0, 0: the luma of the decoded pixel is its Y sample and (I, Q) a fixed
// 2x2 matrix of (Cb, Cr).  So K1 reads the luma plane alone, the compose
// kernels the half-resolution chroma plane alone, and neither goes through
// Pix<FMT> (one interleaved pixel per raw_t).  MM_NV12 and MM_NV12_FULL share
// the instances (FMT = kFmtNV12); their scales and offsets are Geo::nv.
// Alignment: frame base, pitches and the chroma offset are only even
// (mm_surface's unit; tight: rows of W bytes, a frame W H 3/2), so the luma
// plane is read bytewise and a (Cb, Cr) pair as one 2-byte load; dword
// accesses only in the fused kernels' quads, which the host launches for NV12
// only where every row they touch, in every frame of the launch, starts on a
// multiple of 4 (nv12_quads_aligned, mm_impl.hpp: frame bases, strides,
// pitches and chroma offsets of both sides); any other layout takes the
// unfused pair, whose accesses are single samples and pairs.
//
// MM_P010 / MM_P010_FULL (FMT = kFmtP010) are the same layout in little-endian
// 16-bit words, the 10-bit code in the word's high bits (v = word / 64; the low
// 6 bits of a P016 surface are honoured): 2 W bytes per row, 3 W H per frame.
// Every NV12 statement above holds with the word as the sample, Geo::nv in
// word units on input and 10-bit code units on output, and k420<FMT> selects
// the shared 4:2:0 structure of the kernels.  Alignment: frame base, pitches
// and the chroma offset are multiples of 4 (mm_surface's unit), so 2-byte luma
// loads, 4-byte (Cb, Cr) pair loads and 4-byte stores of two words are always
// aligned, and so are the fused kernels' 8-byte quad stores as multi-dword
// accesses (st_stream_pair_a4).
//
// Matrixed frames (a code with MM_MATRIX_BT709 or MM_MATRIX_BT2020): the
// decode's luma weights are not RGBToYIQ's, so the luma of the decoded pixel
// is Yq = y + a cb + b cr (include/mm.h) and K1 reads the pixel's (Cb, Cr) pair
// too.  That is K1's only difference, and its alone: FMT = kFmtNV12M /
// kFmtP010M are K1 instances (both matrices and both ranges share them, a and
// b travel in Geo::nv); the compose kernels read every weight of every 4:2:0
// format from Geo::nv and run the kFmtNV12 / kFmtP010 instances.
constexpr int kFmtNV12 = 16;   // MM_NV12
constexpr int kFmtP010 = 18;   // MM_P010
constexpr int kFmtNV12M = 48;  // MM_NV12 | MM_MATRIX_BT709 (K1 only: any matrixed NV12)
constexpr int kFmtP010M = 50;  // MM_P010 | MM_MATRIX_BT709 (K1 only: any matrixed P010)
template <int FMT> constexpr bool kNV12 = FMT == kFmtNV12 || FMT == kFmtNV12M;
template <int FMT> constexpr bool kP010 = FMT == kFmtP010 || FMT == kFmtP010M;
// three-plane 4:2:0 (MM_I420 = MM_NV12 | MM_PLANAR; section below).  A format
// code past 255 names a pair (fmt_pair), so the template arguments are internal
// codes, NV12's with bit 7: kFmtI420 runs every compose of a three-plane frame,
// kFmtI420M is K1's instance for a matrixed one (a BT.601 frame's K1 is
// kFmtNV12's own: the luma plane is the same plane)
constexpr int kFmtI420 = 144;   // MM_I420* (every range and matrix)
constexpr int kFmtI420M = 176;  // K1 only: any matrixed MM_I420*
template <int FMT> constexpr bool kI420 = FMT == kFmtI420 || FMT == kFmtI420M;
// 10-bit three-plane 4:2:0 (MM_I010 = MM_P010 | MM_PLANAR | MM_LOW_BITS): P010's
// codes with bit 7, in the same roles.  The words hold the code in their LOW 10
// bits (v = word, not word / 64; neither masked nor clamped on input), Cb and Cr
// in planes of their own as in I420, the Cr plane c_pitch x H/2 bytes after the
// Cb plane.  Geo::nv is P010's with the word unit 1 instead of 64 (geo_of): the
// input-side fields differ by exact powers of two, so (float)word - y_off and
// (float)word - 512 are P010's values over 64 exactly and every sum downstream
// scales exactly: a BT.601 frame's K1 is kFmtP010's own instance, and output
// and state are bitwise the P010 path's on the same codes.  The store side is
// P010's codes without the << 6.  Alignment: frame base, pitches, offsets and
// strides are multiples of 2 (mm_surface's unit), so the unfused kernels'
// accesses are single words; the fused kernels' quads (a dword of two Cb words,
// a dword of two Cr words, an 8-byte store of four luma words at a
// dword-aligned address) run only where every row they touch starts on a
// multiple of 4 (i010_quads_aligned, mm_impl.hpp).
constexpr int kFmtI010 = 146;   // MM_I010* (every range and matrix)
constexpr int kFmtI010M = 178;  // K1 only: any matrixed MM_I010*
template <int FMT> constexpr bool kI010 = FMT == kFmtI010 || FMT == kFmtI010M;
template <int FMT> constexpr bool kPlanes3 = kI420<FMT> || kI010<FMT>;   // Cb and Cr planes of their own
template <int FMT> constexpr bool k420 = kNV12<FMT> || kP010<FMT> || kPlanes3<FMT>;
template <int FMT> constexpr bool kMatrixed = FMT == kFmtNV12M || FMT == kFmtP010M || FMT == kFmtI420M || FMT == kFmtI010M;
// packed 4:2:2 (section below): kFmtYUY2 runs every BT.601 YUY2 / UYVY frame and
// every compose, kFmtYUY2M is K1's instance for a matrixed one
constexpr int kFmtYUY2 = 24;   // MM_YUY2
constexpr int kFmtYUY2M = 56;  // MM_YUY2 | MM_MATRIX_BT709 (K1 only: any matrixed packed 4:2:2)
template <int FMT> constexpr bool k422 = FMT == kFmtYUY2 || FMT == kFmtYUY2M;
// 10-bit packed 4:2:2 (section below): kFmtY210 runs every BT.601 Y210 frame and
// every compose, kFmtY210M is K1's instance for a matrixed one
constexpr int kFmtY210 = 22;   // MM_Y210
constexpr int kFmtY210M = 54;  // MM_Y210 | MM_MATRIX_BT709 (K1 only: any matrixed Y210)
template <int FMT> constexpr bool kY210 = FMT == kFmtY210 || FMT == kFmtY210M;
// v210 (section below): the same samples, three 10-bit codes to a dword.  The
// public codes carry MM_PACK_V210 (4096), so the instances are internal codes
// below 256 (22 | 128, 54 | 128), as the three-plane formats' are
constexpr int kFmtV210 = 150;   // MM_V210* (every range and matrix)
constexpr int kFmtV210M = 182;  // K1 only: any matrixed MM_V210*
template <int FMT> constexpr bool kV210 = FMT == kFmtV210 || FMT == kFmtV210M;
// packed RGB (section below): kFmtRGB24 runs every MM_RGB24 and MM_BGR24 frame
constexpr int kFmtRGB24 = 13;  // MM_RGB24
template <int FMT> constexpr bool kRGB24 = FMT == kFmtRGB24;
static_assert(kCodeOut<kFmtRGB24> && kCodeOut<0>, "RGBA8's bytes: composed in code units (yiq_rgba8)");
// Different formats in and out (mm_process_convert): the compose kernels'
// FMT names a PAIR.  A plain format code (< 256) is that format on both sides,
// so the same-format instances keep their names and their code; a mixed pair
// is in | (out + 1) << 8.  Every load-side choice of a compose kernel reads
// kFmtIn<FMT> (the staged raw type, chroma_row / src_iq2, the 4:2:0 sharing of
// chroma rows), every store-side choice kFmtOut<FMT> (the quad store, cd0).
// The ranges and matrices stay uniforms: Geo::nv's (cb, cr) -> (I, Q) fields
// are the input format's, its kr .. cro fields the output format's (geo_of).
constexpr int fmt_pair(int in, int out) { return in | (out + 1) << 8; }
template <int FMT> constexpr int kFmtIn = FMT & 255;
template <int FMT> constexpr int kFmtOut = FMT < 256 ? FMT : (FMT >> 8) - 1;
constexpr int kFmtNV12toRGBA8 = fmt_pair(kFmtNV12, 0);   // decode: MM_NV12* in, MM_RGBA8 out
constexpr int kFmtP010toRGBA8 = fmt_pair(kFmtP010, 0);   // decode: MM_P010* in, MM_RGBA8 out
constexpr int kFmtRGBA8toNV12 = fmt_pair(0, kFmtNV12);   // encode: MM_RGBA8 in, MM_NV12* out
// ... and the same three with MM_BGRA8 as the 4-byte side
constexpr int kFmtNV12toBGRA8 = fmt_pair(kFmtNV12, kFmtBGRA8);
constexpr int kFmtP010toBGRA8 = fmt_pair(kFmtP010, kFmtBGRA8);
constexpr int kFmtBGRA8toNV12 = fmt_pair(kFmtBGRA8, kFmtNV12);
template <int FMT> constexpr bool kFmtPairOk = FMT < 256 || FMT == kFmtNV12toRGBA8 || FMT == kFmtP010toRGBA8 ||
                                               FMT == kFmtRGBA8toNV12 || FMT == kFmtNV12toBGRA8 ||
                                               FMT == kFmtP010toBGRA8 || FMT == kFmtBGRA8toNV12;
// an input macropixel's chroma bytes (byte order: Geo::li.yb; the shifts are uniform)
__device__ __forceinline__ float c422_cb(unsigned u, const Geo &g) { return (float)((u >> (8u - 8u * g.li.yb)) & 255u); }
__device__ __forceinline__ float c422_cr(unsigned u, const Geo &g) { return (float)((u >> (24u - 8u * g.li.yb)) & 255u); }
// (I, Q) of a macropixel's chroma: exact zero for neutral chroma (128, 128)
__device__ __forceinline__ c2 c422_iq2(unsigned u, const Geo &g)
{
    const float cb = c422_cb(u, g) - 128.0f, cr = c422_cr(u, g) - 128.0f;
    return mk(g.nv.icb, g.nv.qcb) * cb + mk(g.nv.icr, g.nv.qcr) * cr;
}
// the raw sample K1 loads per pixel
template <int FMT> struct LumaSrc {
    using raw_t = typename Pix<FMT>::raw_t;
    static constexpr int bpp = Pix<FMT>::bpp;
};
template <> struct LumaSrc<kFmtNV12> {
    using raw_t = uint8_t;
    static constexpr int bpp = 1;
};
// what the compose kernels load per source pixel
template <int FMT> struct ChromaSrc { using raw_t = typename Pix<FMT>::raw_t; };
template <> struct ChromaSrc<kFmtNV12> { using raw_t = uint16_t; };   // Cb | Cr << 8
template <> struct LumaSrc<kFmtP010> {
    using raw_t = uint16_t;
    static constexpr int bpp = 2;
};
template <> struct ChromaSrc<kFmtP010> { using raw_t = uint32_t; };   // Cb | Cr << 16
template <> struct LumaSrc<kFmtNV12M> : LumaSrc<kFmtNV12> {};
template <> struct LumaSrc<kFmtP010M> : LumaSrc<kFmtP010> {};
template <> struct ChromaSrc<kFmtNV12M> : ChromaSrc<kFmtNV12> {};
template <> struct ChromaSrc<kFmtP010M> : ChromaSrc<kFmtP010> {};
// (three-plane: NV12's luma bytes; the pixel's Cb and Cr bytes put together as NV12's pair)
template <> struct LumaSrc<kFmtI420> : LumaSrc<kFmtNV12> {};
template <> struct LumaSrc<kFmtI420M> : LumaSrc<kFmtNV12> {};
template <> struct ChromaSrc<kFmtI420> : ChromaSrc<kFmtNV12> {};
template <> struct ChromaSrc<kFmtI420M> : ChromaSrc<kFmtNV12> {};
// (its 10-bit form: P010's luma words; the pixel's Cb and Cr words put together as P010's pair)
template <> struct LumaSrc<kFmtI010> : LumaSrc<kFmtP010> {};
template <> struct LumaSrc<kFmtI010M> : LumaSrc<kFmtP010> {};
template <> struct ChromaSrc<kFmtI010> : ChromaSrc<kFmtP010> {};
template <> struct ChromaSrc<kFmtI010M> : ChromaSrc<kFmtP010> {};
// K1's luma of a raw sample and its unit (folded into the resample weights)
template <int FMT>
__device__ __forceinline__ float k1_luma(typename LumaSrc<FMT>::raw_t u, const Geo &g)
{
    if constexpr (k420<FMT> || k422<FMT> || kY210<FMT>) return (float)u - g.nv.y_off;
    else return luma_units<FMT>(u);
}
template <int FMT> __device__ __forceinline__ float k1_unit(const Geo &g)
{
    if constexpr (k420<FMT> || k422<FMT> || kY210<FMT> || kV210<FMT>) return g.nv.y_unit;
    else if constexpr (kRGB24<FMT>) return kLumaUnit<0>;   // RGBA8's integer luma
    else return kLumaUnit<FMT>;
}
// A pair of 16-bit words Cb | Cr << 16 as (cb, cr) about the neutral value:
// 0x8000 where the code sits in the word's high bits (P010, MM_Y210), 512 where
// it sits in the low bits (the 10-bit three-plane form; the word is not masked,
// a word above 1023 is that value).  Exactly (0, 0) for neutral chroma.
template <int FMT> constexpr float kWordMid = kI010<FMT> ? 512.0f : 32768.0f;
__device__ __forceinline__ void words_cbcr(unsigned u, float mid, float &cb, float &cr)
{
    cb = (float)(u & 0xFFFFu) - mid, cr = (float)(u >> 16) - mid;
}
// K1, matrixed frames: what a (Cb, Cr) pair adds to the luma of its 2x2
// pixels, in k1_luma's units; exactly 0 for neutral chroma.  One expression
// for the three load forms, so their lumas are bitwise equal.
template <int FMT>
__device__ __forceinline__ float k1_chroma(typename ChromaSrc<FMT>::raw_t u, const Geo &g)
{
    float cb, cr;
    if constexpr (kP010<FMT> || kI010<FMT>) words_cbcr(u, kWordMid<FMT>, cb, cr);
    else if constexpr (k422<FMT>) cb = c422_cb(u, g) - 128.0f, cr = c422_cr(u, g) - 128.0f;
    else cb = (float)(u & 255u) - 128.0f, cr = (float)((unsigned)u >> 8) - 128.0f;
    return fmaf(g.nv.lb, cr, g.nv.la * cb);
}
// K1's chroma plane: row `row` (wrapped or clamped on PIXEL coordinates, then
// halved, as c420_off) and the byte offset of pixel column col's pair in it
template <int FMT> __device__ __forceinline__ const uint8_t *k1_crow(const uint8_t *img, const Geo &g, int row)
{
    return img + (g.li.c_off + (unsigned)(row >> 1) * g.li.c_pitch);
}
template <int FMT> __device__ __forceinline__ unsigned k1_ccol(unsigned col)
{
    return (col & ~1u) * (unsigned)LumaSrc<FMT>::bpp;
}
// Three-plane 4:2:0: the Cr plane lies c_pitch x H/2 bytes after the Cb plane
// (include/mm.h: derived, no Geo field; uniform), and a pixel's (Cb, Cr) is one
// byte of each plane at the same offset, put together as NV12's pair Cb | Cr << 8
__device__ __forceinline__ unsigned i420_cr_delta(const Geo::Lay &l, const Geo &g) { return l.c_pitch * (unsigned)(g.H >> 1); }
__device__ __forceinline__ unsigned i420_ld_pair(const uint8_t *cb, unsigned off, unsigned cr_delta)
{
    return (unsigned)ld_off<uint8_t>(cb, off) | (unsigned)ld_off<uint8_t>(cb, off + cr_delta) << 8;
}
// (the 10-bit form: one word of each plane as P010's pair Cb | Cr << 16; off in bytes)
__device__ __forceinline__ unsigned i010_ld_pair(const uint8_t *cb, unsigned off, unsigned cr_delta)
{
    return (unsigned)ld_off<uint16_t>(cb, off) | (unsigned)ld_off<uint16_t>(cb, off + cr_delta) << 16;
}
// K1's load of pixel column col's (Cb, Cr) from chroma row crow (k1_crow's)
template <int FMT>
__device__ __forceinline__ typename ChromaSrc<FMT>::raw_t k1_cld(const uint8_t *crow, unsigned col, [[maybe_unused]] const Geo &g)
{
    if constexpr (kI420<FMT>) return (uint16_t)i420_ld_pair(crow, col >> 1, i420_cr_delta(g.li, g));
    else if constexpr (kI010<FMT>) return i010_ld_pair(crow, col & ~1u, i420_cr_delta(g.li, g));
    else return ld_off<typename ChromaSrc<FMT>::raw_t>(crow, k1_ccol<FMT>(col));
}
// byte offset of the (Cb, Cr) pair of source pixel (row, col), both already
// wrapped or clamped on PIXEL coordinates (then halved: the decoded frame's
// REPEAT / CLAMP behaviour exactly)
__device__ __forceinline__ unsigned nv12_c_off(const Geo &g, int row, unsigned col)
{
    return g.li.c_off + (unsigned)(row >> 1) * g.li.c_pitch + (col & ~1u);
}
// (I, Q) of a (Cb, Cr) pair: exact zero for neutral chroma (128, 128)
__device__ __forceinline__ c2 nv12_iq2(unsigned u, const Geo &g)
{
    const float cb = (float)(u & 255u) - 128.0f, cr = (float)((u >> 8) & 255u) - 128.0f;
    return mk(g.nv.icb, g.nv.qcb) * cb + mk(g.nv.icr, g.nv.qcr) * cr;
}
// ... and of a pair of 16-bit words about `mid` (words_cbcr): exact zero for neutral chroma
__device__ __forceinline__ c2 word_iq2(unsigned u, float mid, const Geo &g)
{
    float cb, cr;
    words_cbcr(u, mid, cb, cr);
    return mk(g.nv.icb, g.nv.qcb) * cb + mk(g.nv.icr, g.nv.qcr) * cr;
}
__device__ __forceinline__ c2 p010_iq2(unsigned u, const Geo &g) { return word_iq2(u, 32768.0f, g); }
// an MM_Y210 macropixel (dwords Y0 | Cb << 16, Y1 | Cr << 16): its chroma as
// P010's word pair Cb | Cr << 16, and its (I, Q)
__device__ __forceinline__ unsigned y210_cword(uint2 m) { return (m.x >> 16) | (m.y & 0xFFFF0000u); }
__device__ __forceinline__ c2 y210_iq2(uint2 m, const Geo &g) { return p010_iq2(y210_cword(m), g); }
// both for a 4:2:0 format's sample size
template <int FMT> __device__ __forceinline__ unsigned c420_off(const Geo &g, int row, unsigned col)
{
    if constexpr (kP010<FMT>) return g.li.c_off + (unsigned)(row >> 1) * g.li.c_pitch + (col & ~1u) * 2u;
    else if constexpr (kI420<FMT>) return g.li.c_off + (unsigned)(row >> 1) * g.li.c_pitch + (col >> 1);   // (the Cb byte)
    else if constexpr (kI010<FMT>) return g.li.c_off + (unsigned)(row >> 1) * g.li.c_pitch + (col & ~1u);   // (the Cb word)
    else return nv12_c_off(g, row, col);
}
// the (Cb, Cr) pair of source pixel (row, col) as the format's raw pair
template <int FMT> __device__ __forceinline__ unsigned c420_pair(const uint8_t *img, const Geo &g, int row, unsigned col)
{
    if constexpr (kI420<FMT>) return i420_ld_pair(img, c420_off<FMT>(g, row, col), i420_cr_delta(g.li, g));
    else if constexpr (kI010<FMT>) return i010_ld_pair(img, c420_off<FMT>(g, row, col), i420_cr_delta(g.li, g));
    else return ld_off<typename ChromaSrc<FMT>::raw_t>(img, c420_off<FMT>(g, row, col));
}
template <int FMT> __device__ __forceinline__ c2 c420_iq2(unsigned u, const Geo &g)
{
    if constexpr (kP010<FMT> || kI010<FMT>) return word_iq2(u, kWordMid<FMT>, g);
    else return nv12_iq2(u, g);
}
__device__ __forceinline__ c2 rgb24_iq2(uint32_t u, const Geo &g);   // (packed RGB section below)
// the compose kernels' (I, Q) of a staged raw sample
template <int FMT>
__device__ __forceinline__ c2 src_iq2(typename ChromaSrc<FMT>::raw_t u, const Geo &g)
{
    if constexpr (k420<FMT>) return c420_iq2<FMT>(u, g);
    else if constexpr (k422<FMT>) return c422_iq2(u, g);
    else if constexpr (kY210<FMT>) return y210_iq2(u, g);
    else if constexpr (kV210<FMT>) return p010_iq2(u, g);   // (staged as P010's word pair: v210_cword)
    else if constexpr (kRGB24<FMT>) return rgb24_iq2(u, g);
    else return chroma_iq2<FMT>(u);
}
// Output of one pixel from yiq_rgb's saturated RGB: the luma code and the
// unscaled chroma differences (B - Yl, R - Yl) of Y'CbCr.  A 2x2 block's
// chroma code is the rounded scaled sum of its four differences, added as
// (column's two rows) + (neighbour column's two rows) in every kernel, so the
// fused and unfused outputs stay bitwise equal.
__device__ __forceinline__ unsigned nv12_ycode(float r, float gg, float b, const Geo &g, c2 &c)
{
    const float yl = g.nv.kr * r + g.nv.kg * gg + g.nv.kb * b;
    c = mk(b - yl, r - yl);
    return (unsigned)(yl * g.nv.yo_scale + g.nv.yo_bias);   // in 0 .. 255: yl in [0, 1]
}
__device__ __forceinline__ unsigned nv12_ccode(float sum4, float k)
{
    return (unsigned)fminf(sum4 * k + 128.5f, 255.0f);      // >= 1: |C'| <= 1/2
}
// The fused kernels' store of output row i of the quad X .. X+3 (X % 4 == 0;
// rows dword aligned: nv12_quads_aligned): four luma codes as one dword; the even row of a
// row pair leaves its chroma differences in cd0, the odd row adds its own and
// stores the two 2x2 blocks' (Cb, Cr) codes as one dword of chroma row i/2.
__device__ __forceinline__ void nv12_store_quad(uint8_t *outp, const Geo &g, int i, int X, bool odd,
                                                const float (&rr)[4], const float (&gg)[4],
                                                const float (&bb)[4], c2 (&cd0)[4])
{
    c2 cd[4];
    unsigned y4 = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) y4 |= nv12_ycode(rr[k], gg[k], bb[k], g, cd[k]) << (8 * k);
    st_stream<uint32_t>(outp + (size_t)((unsigned)i * g.lo.pitch), (unsigned)X, y4);
    if (!odd) {
#pragma unroll
        for (int k = 0; k < 4; ++k) cd0[k] = cd[k];
    } else {
        const c2 b0 = (cd0[0] + cd[0]) + (cd0[1] + cd[1]), b1 = (cd0[2] + cd[2]) + (cd0[3] + cd[3]);
        const unsigned c4 = nv12_ccode(b0.x, g.nv.cbo) | nv12_ccode(b0.y, g.nv.cro) << 8 |
                            nv12_ccode(b1.x, g.nv.cbo) << 16 | nv12_ccode(b1.y, g.nv.cro) << 24;
        st_stream<uint32_t>(outp + (size_t)(g.lo.c_off + (unsigned)(i >> 1) * g.lo.c_pitch), (unsigned)X, c4);
    }
}
// MM_P010: the same with 10-bit codes (nv12_ycode's is in 0 .. 1023 by the
// range's yo_scale), each stored as code << 6 in a 16-bit word
__device__ __forceinline__ unsigned p010_ccode(float sum4, float k)
{
    return (unsigned)fminf(sum4 * k + 512.5f, 1023.0f);     // >= 1: |C'| <= 1/2
}
// A quad's row is four words, 8 bytes, at a multiple of 8 from the row's start
// (X % 4 == 0); the layout aligns rows to 4 bytes only: one 8-byte store at a
// dword-aligned address (st_stream_pair_a4), in every layout.
__device__ __forceinline__ void p010_st4(uint8_t *row, unsigned X, unsigned lo, unsigned hi)
{
    st_stream_pair_a4(row, X * 2u, lo, hi);
}
__device__ __forceinline__ void p010_store_quad(uint8_t *outp, const Geo &g, int i, int X, bool odd,
                                                const float (&rr)[4], const float (&gg)[4],
                                                const float (&bb)[4], c2 (&cd0)[4])
{
    c2 cd[4];
    unsigned y[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = nv12_ycode(rr[k], gg[k], bb[k], g, cd[k]) << 6;
    p010_st4(outp + (size_t)((unsigned)i * g.lo.pitch), (unsigned)X, y[0] | y[1] << 16, y[2] | y[3] << 16);
    if (!odd) {
#pragma unroll
        for (int k = 0; k < 4; ++k) cd0[k] = cd[k];
    } else {
        const c2 b0 = (cd0[0] + cd[0]) + (cd0[1] + cd[1]), b1 = (cd0[2] + cd[2]) + (cd0[3] + cd[3]);
        const unsigned c0 = p010_ccode(b0.x, g.nv.cbo) << 6 | p010_ccode(b0.y, g.nv.cro) << 22;
        const unsigned c1 = p010_ccode(b1.x, g.nv.cbo) << 6 | p010_ccode(b1.y, g.nv.cro) << 22;
        p010_st4(outp + (size_t)(g.lo.c_off + (unsigned)(i >> 1) * g.lo.c_pitch), (unsigned)X, c0, c1);
    }
}
// Three-plane 4:2:0: nv12_store_quad with the two blocks' Cb codes as one
// 2-byte store to the Cb plane and their Cr codes as one to the Cr plane (X / 2
// is even, chroma rows on multiples of 2: i420_quads_aligned, mm_impl.hpp).
// Same codes, same order of sums.
__device__ __forceinline__ void i420_store_quad(uint8_t *outp, const Geo &g, int i, int X, bool odd,
                                                const float (&rr)[4], const float (&gg)[4],
                                                const float (&bb)[4], c2 (&cd0)[4])
{
    c2 cd[4];
    unsigned y4 = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) y4 |= nv12_ycode(rr[k], gg[k], bb[k], g, cd[k]) << (8 * k);
    st_stream<uint32_t>(outp + (size_t)((unsigned)i * g.lo.pitch), (unsigned)X, y4);
    if (!odd) {
#pragma unroll
        for (int k = 0; k < 4; ++k) cd0[k] = cd[k];
    } else {
        const c2 b0 = (cd0[0] + cd[0]) + (cd0[1] + cd[1]), b1 = (cd0[2] + cd[2]) + (cd0[3] + cd[3]);
        const unsigned cb2 = nv12_ccode(b0.x, g.nv.cbo) | nv12_ccode(b1.x, g.nv.cbo) << 8;
        const unsigned cr2 = nv12_ccode(b0.y, g.nv.cro) | nv12_ccode(b1.y, g.nv.cro) << 8;
        uint8_t *cb = outp + (size_t)(g.lo.c_off + (unsigned)(i >> 1) * g.lo.c_pitch) + ((unsigned)X >> 1);
        __builtin_nontemporal_store((uint16_t)cb2, reinterpret_cast<uint16_t *>(cb));
        __builtin_nontemporal_store((uint16_t)cr2, reinterpret_cast<uint16_t *>(cb + i420_cr_delta(g.lo, g)));
    }
}
// Its 10-bit form: p010_store_quad with the codes unshifted (the word's high 6
// bits zero), the two blocks' Cb codes as one dword store to the Cb plane and
// their Cr codes as one to the Cr plane (X / 2 words is X bytes, X % 4 == 0;
// chroma rows on multiples of 4: i010_quads_aligned, mm_impl.hpp).  Same
// codes, same order of sums.
__device__ __forceinline__ void i010_store_quad(uint8_t *outp, const Geo &g, int i, int X, bool odd,
                                                const float (&rr)[4], const float (&gg)[4],
                                                const float (&bb)[4], c2 (&cd0)[4])
{
    c2 cd[4];
    unsigned y[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = nv12_ycode(rr[k], gg[k], bb[k], g, cd[k]);
    p010_st4(outp + (size_t)((unsigned)i * g.lo.pitch), (unsigned)X, y[0] | y[1] << 16, y[2] | y[3] << 16);
    if (!odd) {
#pragma unroll
        for (int k = 0; k < 4; ++k) cd0[k] = cd[k];
    } else {
        const c2 b0 = (cd0[0] + cd[0]) + (cd0[1] + cd[1]), b1 = (cd0[2] + cd[2]) + (cd0[3] + cd[3]);
        const unsigned cb2 = p010_ccode(b0.x, g.nv.cbo) | p010_ccode(b1.x, g.nv.cbo) << 16;
        const unsigned cr2 = p010_ccode(b0.y, g.nv.cro) | p010_ccode(b1.y, g.nv.cro) << 16;
        uint8_t *cb = outp + (size_t)(g.lo.c_off + (unsigned)(i >> 1) * g.lo.c_pitch);
        st_stream<uint32_t>(cb, (unsigned)X, cb2);
        st_stream<uint32_t>(cb + i420_cr_delta(g.lo, g), (unsigned)X, cr2);
    }
}
// the fused kernels' quad store for a 4:2:0 format
template <int FMT>
__device__ __forceinline__ void c420_store_quad(uint8_t *outp, const Geo &g, int i, int X, bool odd,
                                                const float (&rr)[4],
                                                const float (&gg)[4], const float (&bb)[4], c2 (&cd0)[4])
{
    if constexpr (kP010<FMT>) p010_store_quad(outp, g, i, X, odd, rr, gg, bb, cd0);
    else if constexpr (kI420<FMT>) i420_store_quad(outp, g, i, X, odd, rr, gg, bb, cd0);
    else if constexpr (kI010<FMT>) i010_store_quad(outp, g, i, X, odd, rr, gg, bb, cd0);
    else nv12_store_quad(outp, g, i, X, odd, rr, gg, bb, cd0);
}
// the fused kernels' load of the two (Cb, Cr) pairs of the quad X .. X+3 in
// source row `row`
template <int FMT>
__device__ __forceinline__ void c420_quad_pairs(const uint8_t *img, const Geo &g, int row, unsigned X,
                                                unsigned &p0, unsigned &p1)
{
    if constexpr (kP010<FMT>) {   // two 4-byte loads: rows are 4-byte aligned only
        p0 = ld_off<uint32_t>(img, c420_off<FMT>(g, row, X));
        p1 = ld_off<uint32_t>(img, c420_off<FMT>(g, row, X) + 4u);
    } else if constexpr (kI420<FMT>) {   // one 2-byte load per plane (chroma rows on multiples of 2, X / 2 even)
        const unsigned off = c420_off<FMT>(g, row, X);
        const unsigned cb2 = ld_off<uint16_t>(img, off), cr2 = ld_off<uint16_t>(img, off + i420_cr_delta(g.li, g));
        p0 = (cb2 & 255u) | (cr2 & 255u) << 8;
        p1 = (cb2 >> 8) | (cr2 >> 8) << 8;
    } else if constexpr (kI010<FMT>) {   // one dword per plane (chroma rows on multiples of 4, X / 2 words = X bytes)
        const unsigned off = c420_off<FMT>(g, row, X);
        const unsigned cb2 = ld_off<uint32_t>(img, off), cr2 = ld_off<uint32_t>(img, off + i420_cr_delta(g.li, g));
        p0 = (cb2 & 0xFFFFu) | cr2 << 16;
        p1 = (cb2 >> 16) | (cr2 & 0xFFFF0000u);
    } else {                      // one dword (rows dword aligned: nv12_quads_aligned)
        p0 = ld_off<uint32_t>(img, nv12_c_off(g, row, X));
        p1 = p0 >> 16;
    }
}

// ---- single-plane grayscale (MM_Y8 .. MM_Y16) ------------------------------
// A frame is H rows of W samples, bytes (MM_Y8) or little-endian 16-bit words
// with the code in the low bits (MM_Y10 / MM_Y12 / MM_Y16).  It IS the RGBA32F
// frame R = G = B = v = sample / max, alpha 1 (include/mm.h): the luma of the
// pixel is the sample and (I, Q) is zero.  So K1 is the luma-plane path of the
// 4:2:0 formats with other uniforms, and it runs THEIR instances (kFmtNV12 for
// bytes, kFmtP010 for words, the GEN form included, which the 4:2:0 formats
// themselves never launch): with y_off = 0 their (float)sample - y_off is
// (float)sample bit for bit, and y_unit = 1 / max folds into the resample
// weights as NV12's 1 / 219 does.  The compose kernels have instances of their
// own (FMT = kFmtY8, kFmtY16; the three word depths share one, Geo::nv.yo_scale
// = max tells them apart) that never read the input frame: with zero (I, Q)
// YIQToRGB gives R = G = B = sat(Y'), whose luma is sat(Y') itself, so a pixel
// is vertical blur -> sat -> code -> store, the blur written as in every other
// instance.  No chroma subsampling: odd sizes and the debug views (the view's
// R value is the sample) are supported.
// Alignment: frame base, pitch and stride are multiples of the sample size
// only, so the unfused kernels store single samples; the fused kernels' quad
// (four bytes as one dword, four words as one 8-byte store at a dword-aligned
// address) runs only where every output row of the launch starts on a multiple
// of 4 (mono_quads_aligned, mm_impl.hpp).
constexpr int kFmtY8 = 8;     // MM_Y8
constexpr int kFmtY16 = 11;   // MM_Y16 (and MM_Y10, MM_Y12)
template <int FMT> constexpr bool kMono = FMT == kFmtY8 || FMT == kFmtY16;
template <> struct LumaSrc<kFmtY8> : LumaSrc<kFmtNV12> {};
template <> struct LumaSrc<kFmtY16> : LumaSrc<kFmtP010> {};
template <> struct ChromaSrc<kFmtY8> { using raw_t = uint32_t; };    // (never loaded)
template <> struct ChromaSrc<kFmtY16> { using raw_t = uint32_t; };
// code of a saturated value v in [0, 1]: floor(v max + 0.5), at most max
__device__ __forceinline__ unsigned mono_code(float v, const Geo &g)
{
    return (unsigned)fminf(v * g.nv.yo_scale + g.nv.yo_bias, g.nv.yo_scale);
}
// one sample of row `row` (the unfused, odd-size and debug kernels)
template <int FMT>
__device__ __forceinline__ void mono_store(uint8_t *row, unsigned X, float v, const Geo &g)
{
    if constexpr (FMT == kFmtY8) st_off<uint8_t>(row, X, (uint8_t)mono_code(v, g));
    else st_off<uint16_t>(row, X * 2u, (uint16_t)mono_code(v, g));
}
// the fused kernels' quad X .. X+3 (X % 4 == 0) of a dword-aligned row
template <int FMT>
__device__ __forceinline__ void mono_store_quad(uint8_t *row, unsigned X, const float (&v)[4], const Geo &g)
{
    unsigned c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = mono_code(v[k], g);
    if constexpr (FMT == kFmtY8) st_stream<uint32_t>(row, X, c[0] | c[1] << 8 | c[2] << 16 | c[3] << 24);
    else st_stream_pair_a4(row, X * 2u, c[0] | c[1] << 16, c[2] | c[3] << 16);
}

// ---- packed RGB (MM_RGB24 / MM_BGR24) access -------------------------------
// A frame is H rows of W three-byte pixels, bytes R G B (MM_RGB24) or B G R
// (MM_BGR24), UNORM as MM_RGBA8's and no alpha byte.  It IS the MM_RGBA8 frame
// with the same colour bytes and alpha 255 (include/mm.h), and the operator
// gives the alpha byte weight 0 everywhere, so every value is computed by
// MM_RGBA8's own expressions (luma_units<0>'s integer, chroma_iq2<0>,
// Pix<0>::pack) and the output bytes and the state are bitwise that frame's:
// a 3-byte pixel is an addressing problem.  Both byte orders share the one
// instance of every kernel (FMT = kFmtRGB24); the order travels in Geo::li.yb /
// lo.yb (0: R first, 1: B first), where packed 4:2:2 keeps its own, and turns
// into uniform operands: K1's two dot weights, the compose's byte selectors.
//   Loads of one pixel (K1, the unfused, odd-size kernels, the fused kernels'
//     two outer columns): ONE byte-aligned dword at 3 col, whose fourth byte is
//     the next pixel's first and is never used (weight 0 in K1's dots, dropped
//     by the selector elsewhere).  The row's last pixel is loaded one byte
//     earlier and shifted down 8, so no byte outside the row's 3 W is touched
//     (W >= 2).  Three lanes in four are misaligned; global memory takes that.
//     (The other form, two aligned dwords and v_alignbyte_b32, was built and
//     measured in K1: the same time per 1080p frame, 5.3-5.4 us, with twice
//     the loads, 90 VGPRs for 57 at N = 2048 and 19 spilled at N = 8192.  Not
//     kept.  DESIGN.md, "Packed RGB frames".)
//   K1: the luma is RGBA8's exact integer 299 R + 587 G + 114 B by the same two
//     v_dot4_u32_u8, the weights in the frame's byte order (R G B: 0x00000201
//     and 0x00724B2B; B G R: 0x00010200 and 0x002B4B72), so every form (regular,
//     shared rows, LAT, GEN) has the RGBA8 instance's lumas bit for bit.
//   compose: a pixel's R, G, B come out of the loaded dword(s) by one v_perm_b32
//     with a uniform selector as the RGBA8 word R | G << 8 | B << 16 and go
//     through chroma_iq2<0>; results are packed by Pix<0>::pack and leave
//     through the same permute.  The fused kernels' quad X .. X+3 (X % 4 == 0)
//     is 12 bytes at 3 X: one dwordx3 load and one non-temporal dwordx3 store,
//     typed 4-byte aligned like RGBA8's quads (ld_quad_a4), which the host
//     launches only where every row of the launch starts on a multiple of 4
//     on both sides (rgb24_quads_aligned, mm_impl.hpp; any other layout takes
//     the unfused pair).  The unfused kernels store a pixel as three bytes.
// The unit is 1: base, pitch and stride are any bytes.  No subsampling: odd
// sizes and the debug views (R = the view's value, G = B = 0, as RGBA8's) are
// supported.  The LDS-DMA source staging stays RGBA8's (4-byte pixels).
template <> struct LumaSrc<kFmtRGB24> {    // the dword that starts at the pixel
    using raw_t = uint32_t;
    static constexpr int bpp = 3;
};
template <> struct ChromaSrc<kFmtRGB24> { using raw_t = uint32_t; };
typedef uint32_t u32_a1 __attribute__((aligned(1)));
typedef unsigned u32x3_a4 __attribute__((ext_vector_type(3), aligned(4)));
// byte offset in its row of the dword loaded for pixel column col, and the
// pixel (its three bytes in the low 24 bits) of that dword
__device__ __forceinline__ unsigned rgb24_off(unsigned col, const Geo &g)
{
    return 3u * col - (col == (unsigned)(g.W - 1) ? 1u : 0u);
}
__device__ __forceinline__ uint32_t rgb24_fix(uint32_t u, unsigned col, const Geo &g)
{
    return col == (unsigned)(g.W - 1) ? u >> 8 : u;
}
__device__ __forceinline__ uint32_t rgb24_px(const void *row, unsigned row_off, unsigned col, const Geo &g)
{
    const uint32_t u = *reinterpret_cast<const u32_a1 *>(reinterpret_cast<const uint8_t *>(row) + (row_off + rgb24_off(col, g)));
    return rgb24_fix(u, col, g);
}
// K1: luma_units<0>'s integer of a pixel in the frame's byte order
__device__ __forceinline__ float rgb24_luma_units(uint32_t u, const Geo &g)
{
    const unsigned w0 = g.li.yb ? 0x00010200u : 0x00000201u, w1 = g.li.yb ? 0x002B4B72u : 0x00724B2Bu;
    const unsigned hi = __builtin_amdgcn_udot4(u, w0, 0u, false);     // R + 2 G
    return (float)__builtin_amdgcn_udot4(u, w1, hi << 8, false);      // + 43 R + 75 G + 114 B
}
// v_perm_b32 selector of three bytes that start at byte `pos` of the pair
// (hi : lo), as R | G << 8 | B << 16 (top byte 0) for byte order yb, and the
// reverse for pos = 0: the frame's three bytes of an RGBA8 word
__device__ __forceinline__ unsigned rgb24_sel(unsigned pos, unsigned yb)
{
    return 0x0C000000u | (pos + 1u) << 8 | (yb ? pos << 16 | (pos + 2u) : (pos + 2u) << 16 | pos);
}
// the RGBA8 word (alpha byte 0, never used) of a loaded pixel, and its (I, Q)
__device__ __forceinline__ uint32_t rgb24_canon(uint32_t u, const Geo &g)
{
    return __builtin_amdgcn_perm(u, u, rgb24_sel(0u, g.li.yb));
}
__device__ __forceinline__ c2 rgb24_iq2(uint32_t u, const Geo &g) { return chroma_iq2<0>(rgb24_canon(u, g)); }
// one output pixel of row `row`: its RGBA8 word's bytes in the frame's order,
// three byte stores (rgb24_store_px: the unfused compose, the word from
// yiq_rgba8; rgb24_store: the odd-size and debug kernels, from Pix<0>::pack)
__device__ __forceinline__ void rgb24_store_px(uint8_t *row, unsigned X, uint32_t px, const Geo &g)
{
    const uint32_t q = __builtin_amdgcn_perm(0u, px, rgb24_sel(0u, g.lo.yb));
    st_off<uint8_t>(row, 3u * X, (uint8_t)q);
    st_off<uint8_t>(row, 3u * X + 1u, (uint8_t)(q >> 8));
    st_off<uint8_t>(row, 3u * X + 2u, (uint8_t)(q >> 16));
}
__device__ __forceinline__ void rgb24_store(uint8_t *row, unsigned X, float r, float gg, float b, const Geo &g)
{
    rgb24_store_px(row, X, Pix<0>::pack(r, gg, b), g);
}
// The fused kernels' (I, Q) of source columns X-1 .. X+4 (cl, cr: the outer
// two, wrapped or clamped) of source row `row`: the quad's 12 bytes as one load
__device__ __forceinline__ void rgb24_quad_iq(const uint8_t *img, const Geo &g, int row, unsigned X, unsigned cl,
                                              unsigned cr, c2 (&a)[6])
{
    const unsigned ro = (unsigned)row * g.li.pitch;
    const uint32_t pl = rgb24_px(img, ro, cl, g);
    const u32x3_a4 m = *reinterpret_cast<const u32x3_a4 *>(img + (ro + 3u * X));
    const uint32_t pr = rgb24_px(img, ro, cr, g);
    const unsigned yb = g.li.yb;
    a[0] = rgb24_iq2(pl, g);
    a[1] = chroma_iq2<0>(__builtin_amdgcn_perm(m.x, m.x, rgb24_sel(0u, yb)));   // bytes 0 .. 2
    a[2] = chroma_iq2<0>(__builtin_amdgcn_perm(m.y, m.x, rgb24_sel(3u, yb)));   // 3 .. 5
    a[3] = chroma_iq2<0>(__builtin_amdgcn_perm(m.z, m.y, rgb24_sel(2u, yb)));   // 6 .. 8
    a[4] = chroma_iq2<0>(__builtin_amdgcn_perm(m.z, m.z, rgb24_sel(1u, yb)));   // 9 .. 11
    a[5] = rgb24_iq2(pr, g);
}
// The fused kernels' store of output row i of the quad X .. X+3 (X % 4 == 0):
// four packed pixels as 12 bytes, one non-temporal store at a dword-aligned
// address.  Byte j of output pixel k is byte c(j) of its RGBA8 word, c(j) = j
// (R G B) or 2 - j (B G R).
// (p: the four pixels' RGBA8 words, the compose's yiq_rgba8)
__device__ __forceinline__ void rgb24_store_quad(uint8_t *outp, const Geo &g, int i, int X, const uint32_t (&p)[4])
{
    const bool sw = g.lo.yb != 0;
    u32x3_a4 w;
    w.x = __builtin_amdgcn_perm(p[1], p[0], sw ? 0x06000102u : 0x04020100u);   // c0 c1 c2 | c0
    w.y = __builtin_amdgcn_perm(p[2], p[1], sw ? 0x05060001u : 0x05040201u);   // c1 c2 | c0 c1
    w.z = __builtin_amdgcn_perm(p[3], p[2], sw ? 0x04050600u : 0x06050402u);   // c2 | c0 c1 c2
    unsigned off = (unsigned)X * 3u;
    __builtin_nontemporal_store(w, reinterpret_cast<u32x3_a4 *>(outp + (size_t)((unsigned)i * g.lo.pitch) + off));
}

// ---- packed 4:2:2 (MM_YUY2 / MM_UYVY) access -------------------------------
// A frame is one plane of H rows of W / 2 four-byte macropixels, Y0 Cb Y1 Cr
// (YUY2) or Cb Y0 Cr Y1 (UYVY): two pixels that share one (Cb, Cr) pair; W and
// H even.  It IS the RGBA32F frame its decode gives (include/mm.h), with NV12's
// codes and ranges and the matrix bits' matrices, so every statement of the
// NV12 section holds with "its 1 x 2 pixels" for "its 2 x 2 pixels".  Both byte
// orders, both ranges and all three matrices share the instances: the byte
// order travels in Geo::li.yb / lo.yb (Y0's byte; Cb's is the other one, Y1
// and Cr lie 16 bits above), the ranges and matrices in Geo::nv where the
// 4:2:0 formats keep them.
//   K1, BT.601 (FMT = kFmtYUY2): the luma of the decoded pixel is its Y byte,
//     at a byte stride of 2.  A lane loads the aligned 16-bit (Y, C) pair of
//     its pixel, so that a wave's loads are contiguous like a P010 luma
//     row's (the Y bytes alone, as byte loads at stride 2, ran K1 at 5.3-5.5
//     us per 1080p frame against 4.3 for the matrixed instance's dwords), and
//     keeps the Y byte by a uniform shift; the chroma byte is never used.
//     k1_luma's expression and the packed V2 expressions are the kFmtNV12
//     instance's: the state is bitwise an NV12 frame's with the same luma
//     samples.
//   K1, matrixed (FMT = kFmtYUY2M): one aligned dword per pixel and source row
//     is the pixel's macropixel: Y by the column's parity, Cb and Cr through
//     k1_chroma's one expression (neutral chroma adds exactly 0).  No second
//     plane, no k1_crow.
//   compose (FMT = kFmtYUY2, all three forms): source columns X-1 .. X+4 of
//     the quad X .. X+3 are macropixels X/2-1 .. X/2+2, the outer two wrapped
//     or clamped on PIXEL coordinates and then halved (dword loads), the
//     quad's own two one 8-byte load.  Every output row has its own source
//     rows: the RGBA formats' row schedule.  A chroma code is the scaled sum
//     (left pixel's difference + right pixel's difference), formed that way in
//     every kernel, so the fused and unfused outputs stay bitwise equal; a row
//     of the quad leaves as two whole macropixels in one 8-byte store, the
//     unfused k_compose's even lanes store one macropixel each (the lane pair
//     exchanges one chroma difference and one 16-bit half).  No thread
//     writes part of a macropixel.
// Alignment: frame base, pitch and stride are multiples of 4 (mm_surface's
// unit, one macropixel), so every dword access is aligned in every legal
// layout and the 8-byte quads are multi-dword accesses at dword-aligned
// addresses (ld_pair_a4 / st_stream_pair_a4): no layout rule of its own for
// the fused kernels.  No GEN, k_compose_odd or k_dbg_out instance: odd sizes
// and the debug views are refused on the host.
template <> struct LumaSrc<kFmtYUY2> {     // the pixel's (Y, C) byte pair
    using raw_t = uint16_t;
    static constexpr int bpp = 2;
};
template <> struct LumaSrc<kFmtYUY2M> {    // the pixel's whole macropixel
    using raw_t = uint32_t;
    static constexpr int bpp = 2;
};
template <> struct ChromaSrc<kFmtYUY2> { using raw_t = uint32_t; };    // the macropixel
template <> struct ChromaSrc<kFmtYUY2M> { using raw_t = uint32_t; };
// ---- v210 (MM_V210) access ---------------------------------------------------
// MM_Y210's samples, three 10-bit codes to a little-endian dword (bits 0-9,
// 10-19, 20-29; bits 30-31 unused) and six pixels to a group of four dwords:
//   dword 0: Cb(0,1) Y0 Cr(0,1)   dword 1: Y1 Cb(2,3) Y2
//   dword 2: Cr(2,3) Y3 Cb(4,5)   dword 3: Y4 Cr(4,5) Y5
// A frame IS the MM_Y210 frame whose words are code << 6: every code read here
// enters the Y210 / P010 expressions as that word, so state and output codes
// are bitwise the Y210 path's.  Column c = col % 6 of group q = col / 6 (a
// multiply-high, no integer divide); pixel pair p = c / 2.
//   K1, BT.601 (kFmtV210): one aligned dword per tap, dword 4 q + {0, 1, 1, 2,
//     3, 3}[c], field at bit {10, 0, 20, 10, 0, 20}[c].
//   K1, matrixed (kFmtV210M), and the compose's source side: the two dwords
//     p, p + 1 of the group hold the pair's Cb, Cr and both its lumas (one
//     8-byte load at a dword-aligned address: pair 1 starts at byte 4).  With
//     v = d[p] | d[p+1] << 32: Cb at bit 10 p, Cr at bit {20, 32, 42}[p], Y at
//     bit {10, 32, 20, 42, 32, 52}[c].  Eight bytes per tap, as the Y210
//     instance loads (a whole group per tap, 16 bytes: twice the registers of
//     the load batch).
//   compose, store side (k_compose with tiles of kTileColsG columns): a lane holds its pixel's luma code and
//     its pair's Cb (even lane) or Cr (odd lane) code; a dword mixes the codes
//     of up to three lanes, so the codes of a tile go through LDS and the first
//     lane of each group stores the group: one aligned 16-byte store, or the 8
//     or 12 bytes of a partial last group (W % 6 = 2, 4), unused fields zero.
// Alignment: frame base, pitch and stride are multiples of 16 (mm_surface's
// unit, one group), so every group is 16-byte aligned in every legal layout.
// No fused K34, GEN, k_compose_odd, k_dbg_out or k_convert instance.
template <> struct LumaSrc<kFmtV210> {     // the dword that holds the pixel's luma
    using raw_t = uint32_t;
    static constexpr int bpp = 0;          // (no bytes per pixel: k1_off)
};
template <> struct LumaSrc<kFmtV210M> {    // the pair's two dwords
    using raw_t = uint2;
    static constexpr int bpp = 0;
};
template <> struct ChromaSrc<kFmtV210> { using raw_t = uint32_t; };    // P010's word pair Cb << 6 | Cr << 22
template <> struct ChromaSrc<kFmtV210M> { using raw_t = uint32_t; };
__device__ __forceinline__ unsigned v210_group(unsigned col) { return __umulhi(col, 0xAAAAAAABu) >> 2; }   // col / 6
// byte offset in the row of the dword that holds column col's luma
__device__ __forceinline__ unsigned v210_y_off(unsigned col)
{
    const unsigned q = v210_group(col), c = col - 6u * q;
    return 16u * q + 4u * ((0x332110u >> (4u * c)) & 3u);
}
__device__ __forceinline__ unsigned v210_y_shift(unsigned col)
{
    const unsigned c = col - 6u * v210_group(col);
    return 10u * ((0x861u >> (2u * c)) & 3u);
}
// ... of the pair's two dwords
__device__ __forceinline__ unsigned v210_pair_off(unsigned col)
{
    const unsigned q = v210_group(col), c = col - 6u * q;
    return 16u * q + 4u * (c >> 1);
}
// the pair's two dwords (v210_pair_off's) -> column col's luma code, the pair's
// chroma as P010's word pair
__device__ __forceinline__ unsigned v210_pair_y(uint2 m, unsigned col)
{
    const unsigned c = col - 6u * v210_group(col);
    const unsigned long long v = (unsigned long long)m.y << 32 | m.x;
    // bit {10, 32, 20, 42, 32, 52}[c], one byte each
    return (unsigned)(v >> ((0x34202A14200Aull >> (8u * c)) & 63u)) & 1023u;
}
__device__ __forceinline__ unsigned v210_cword(uint2 m, unsigned col)
{
    const unsigned p = (col - 6u * v210_group(col)) >> 1;
    const unsigned long long v = (unsigned long long)m.y << 32 | m.x;
    const unsigned cb = (unsigned)(v >> (10u * p)) & 1023u;
    const unsigned cr = (unsigned)(v >> ((0x2A2014u >> (8u * p)) & 63u)) & 1023u;   // bit {20, 32, 42}[p]
    return cb << 6 | cr << 22;
}
// One group of an output row from the six lanes' codes e[k] = Y | C << 16 (C:
// Cb of an even, Cr of an odd column), `n` of them inside the frame (2, 4, 6)
__device__ __forceinline__ void v210_store_group(uint8_t *row, unsigned group, const unsigned (&e)[6], int n)
{
    const unsigned d0 = e[0] >> 16 | (e[0] & 1023u) << 10 | (e[1] >> 16) << 20;
    const unsigned d1 = (e[1] & 1023u) | (e[2] >> 16) << 10 | (e[2] & 1023u) << 20;
    const unsigned d2 = e[3] >> 16 | (e[3] & 1023u) << 10 | (e[4] >> 16) << 20;
    const unsigned d3 = (e[4] & 1023u) | (e[5] >> 16) << 10 | (e[5] & 1023u) << 20;
    if (n == 6) {
        st_stream<uint4>(row, group * 16u, make_uint4(d0, d1, d2, d3));
    } else {
        st_stream<uint2>(row, group * 16u, make_uint2(d0, d1));
        if (n == 4) st_stream<uint32_t>(row, group * 16u + 8u, d2);
    }
}

// K1: byte offset of pixel column col's sample in its source row
template <int FMT> __device__ __forceinline__ unsigned k1_off(unsigned col)
{
    if constexpr (FMT == kFmtYUY2M) return (col & ~1u) * 2u;
    else if constexpr (FMT == kFmtY210M) return (col & ~1u) * 4u;
    else if constexpr (FMT == kFmtV210) return v210_y_off(col);
    else if constexpr (FMT == kFmtV210M) return v210_pair_off(col);
    else return col * (unsigned)LumaSrc<FMT>::bpp;
}
// ... of the load for pixel column col (packed RGB: the row's last pixel is
// loaded one byte earlier, rgb24_off)
template <int FMT> __device__ __forceinline__ unsigned k1_off(unsigned col, [[maybe_unused]] const Geo &g)
{
    if constexpr (kRGB24<FMT>) return rgb24_off(col, g);
    else return k1_off<FMT>(col);
}
// K1's load of a sample (packed RGB: a dword at any byte)
template <int FMT> __device__ __forceinline__ typename LumaSrc<FMT>::raw_t k1_ld(const void *row, unsigned off)
{
    // (the typedef itself: a template argument would drop its alignment)
    if constexpr (kRGB24<FMT>) return *reinterpret_cast<const u32_a1 *>(reinterpret_cast<const uint8_t *>(row) + off);
    else if constexpr (FMT == kFmtV210M) return ld_pair_a4(row, off);   // (pair 1 of a group starts at byte 4)
    else return ld_off<typename LumaSrc<FMT>::raw_t>(row, off);
}
// K1: the luma of column col's loaded sample (in k1_luma's units).  One
// expression for the three load forms.
template <int FMT>
__device__ __forceinline__ float k1_luma_at(typename LumaSrc<FMT>::raw_t u, [[maybe_unused]] unsigned col, const Geo &g)
{
    if constexpr (FMT == kFmtYUY2M) {
        const unsigned yc = (u >> (8u * g.li.yb + ((col & 1u) << 4))) & 255u;
        return k1_luma<FMT>(yc, g) + k1_chroma<FMT>(u, g);
    } else if constexpr (FMT == kFmtYUY2) {
        return k1_luma<FMT>((uint16_t)(((unsigned)u >> (8u * g.li.yb)) & 255u), g);
    } else if constexpr (FMT == kFmtY210M) {
        const unsigned yc = (col & 1u ? u.y : u.x) & 0xFFFFu;
        return k1_luma<kFmtP010M>((uint16_t)yc, g) + k1_chroma<kFmtP010M>(y210_cword(u), g);
    } else if constexpr (FMT == kFmtY210) {
        return k1_luma<kFmtP010>((uint16_t)(u & 0xFFFFu), g);
    } else if constexpr (FMT == kFmtV210M) {
        // (the Y210 instance's expression on the words code << 6)
        return k1_luma<kFmtP010M>((uint16_t)(v210_pair_y(u, col) << 6), g) + k1_chroma<kFmtP010M>(v210_cword(u, col), g);
    } else if constexpr (FMT == kFmtV210) {
        return k1_luma<kFmtP010>((uint16_t)(((u >> v210_y_shift(col)) & 1023u) << 6), g);
    } else if constexpr (kRGB24<FMT>) {
        return rgb24_luma_units(rgb24_fix(u, col, g), g);
    } else {
        return k1_luma<FMT>(u, g);
    }
}
// byte offset of the macropixel of source pixel (row, col), both already
// wrapped or clamped on PIXEL coordinates (then halved)
__device__ __forceinline__ unsigned c422_off(const Geo &g, int row, unsigned col)
{
    return (unsigned)row * g.li.pitch + (col >> 1) * 4u;
}
// One output macropixel: its two luma codes and the sum of its two pixels'
// chroma differences (nv12_ycode's; cbo, cro hold the mean's 1/2)
__device__ __forceinline__ unsigned c422_pack(unsigned y0, unsigned y1, c2 sum2, const Geo &g)
{
    const unsigned c = nv12_ccode(sum2.x, g.nv.cbo) | nv12_ccode(sum2.y, g.nv.cro) << 16;
    return (y0 | y1 << 16) << (8u * g.lo.yb) | c << (8u - 8u * g.lo.yb);
}
// The fused kernels' store of output row i of the quad X .. X+3 (X % 4 == 0):
// two macropixels as one 8-byte store at a dword-aligned address
__device__ __forceinline__ void c422_store_quad(uint8_t *outp, const Geo &g, int i, int X, const float (&rr)[4],
                                                const float (&gg)[4], const float (&bb)[4])
{
    c2 cd[4];
    unsigned y[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = nv12_ycode(rr[k], gg[k], bb[k], g, cd[k]);
    st_stream_pair_a4(outp + (size_t)((unsigned)i * g.lo.pitch), (unsigned)X * 2u,
                      c422_pack(y[0], y[1], cd[0] + cd[1], g), c422_pack(y[2], y[3], cd[2] + cd[3], g));
}
// The fused kernels' (I, Q) of source columns X-1 .. X+4 (cl, cr: the outer two,
// wrapped or clamped) of source row `row`
__device__ __forceinline__ void c422_quad_iq(const uint8_t *img, const Geo &g, int row, unsigned X, unsigned cl,
                                             unsigned cr, c2 (&a)[6])
{
    const unsigned pl = ld_off<uint32_t>(img, c422_off(g, row, cl));
    const uint2 pm = ld_pair_a4(img, c422_off(g, row, X));
    const unsigned pr = ld_off<uint32_t>(img, c422_off(g, row, cr));
    a[0] = c422_iq2(pl, g);
    a[1] = a[2] = c422_iq2(pm.x, g);
    a[3] = a[4] = c422_iq2(pm.y, g);
    a[5] = c422_iq2(pr, g);
}

// ---- 10-bit packed 4:2:2 (MM_Y210) access ----------------------------------
// A frame is one plane of H rows of W / 2 eight-byte macropixels: four
// little-endian 16-bit words Y0 Cb Y1 Cr, the 10-bit code in the word's high
// bits as in P010 (v = word / 64; the low 6 bits of a Y216 surface are
// honoured).  It IS the RGBA32F frame its decode gives (include/mm.h), with
// P010's codes and ranges and the matrix bits' matrices; every statement of the
// packed 4:2:2 section holds with the word as the sample and Geo::nv as P010
// has it (word units in, 10-bit code units out, the mean of two).  There is
// one word order (Geo::li.yb / lo.yb stay 0).
//   K1, BT.601 (FMT = kFmtY210): a lane loads the aligned dword (Y, C) of its
//     pixel, so that a wave's loads are contiguous, and keeps the low word;
//     k1_luma's expression and the packed V2 expressions are the kFmtP010
//     instance's: the state is bitwise a P010 frame's with the same luma words.
//   K1, matrixed (FMT = kFmtY210M): one aligned 8-byte load per pixel and source
//     row is the pixel's macropixel, dwords Y0 | Cb << 16 and Y1 | Cr << 16: Y
//     by the column's parity, and (d0 >> 16) | (d1 & 0xffff0000) is P010's
//     chroma word Cb | Cr << 16, which goes through k1_chroma's P010 expression
//     (neutral chroma, 0x8000, adds exactly 0).
//   compose (FMT = kFmtY210, all three forms): the schedule of the 8-bit form
//     with 8-byte macropixels.  The outer source columns X-1 and X+4 are 8-byte
//     loads, the quad's own two macropixels one 16-byte load; a row of the quad
//     leaves as two whole macropixels in one 16-byte store, the unfused
//     k_compose's even lanes store one macropixel (8 bytes) each.  Codes are
//     P010's (nv12_ycode by the range's scale, p010_ccode), stored << 6.
// Alignment: frame base, pitch and stride are multiples of 8 (mm_surface's
// unit, one macropixel), so every 8-byte access is aligned in every legal
// layout.  The 16-byte quads lie at multiples of 16 from the row's start (X % 4
// == 0): 16-byte aligned wherever base, pitch and stride are (every tight frame
// with W % 4 == 0, every decoder layout), and multi-dword accesses at
// 8-byte-aligned addresses otherwise (ld_quad_a8 / st_stream_quad_a8, as
// RGBA8's quads at dword-aligned ones): one access in every layout, no layout
// rule of its own for the fused kernels.  No GEN, k_compose_odd or k_dbg_out
// instance: odd sizes and the debug views are refused on the host.
template <> struct LumaSrc<kFmtY210> {     // the pixel's (Y, C) word pair
    using raw_t = uint32_t;
    static constexpr int bpp = 4;
};
template <> struct LumaSrc<kFmtY210M> {    // the pixel's whole macropixel
    using raw_t = uint2;
    static constexpr int bpp = 4;
};
template <> struct ChromaSrc<kFmtY210> { using raw_t = uint2; };    // the macropixel
template <> struct ChromaSrc<kFmtY210M> { using raw_t = uint2; };
// byte offset of the macropixel of source pixel (row, col), both already
// wrapped or clamped on PIXEL coordinates (then halved)
__device__ __forceinline__ unsigned y210_off(const Geo &g, int row, unsigned col)
{
    return (unsigned)row * g.li.pitch + (col >> 1) * 8u;
}
// One word pair of an output macropixel: a luma code and a chroma code (of the
// sum of the macropixel's two chroma differences; cbo, cro hold the mean's 1/2)
__device__ __forceinline__ unsigned y210_half(unsigned y, float sum2, float k)
{
    return y << 6 | p010_ccode(sum2, k) << 22;
}
// The fused kernels' store of output row i of the quad X .. X+3 (X % 4 == 0):
// two macropixels as one 16-byte store
__device__ __forceinline__ void y210_store_quad(uint8_t *outp, const Geo &g, int i, int X, const float (&rr)[4],
                                                const float (&gg)[4], const float (&bb)[4])
{
    c2 cd[4];
    unsigned y[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = nv12_ycode(rr[k], gg[k], bb[k], g, cd[k]);
    const c2 s0 = cd[0] + cd[1], s1 = cd[2] + cd[3];
    // (the column offset formed here, per row: hoisted out of the walking
    // kernel's row loop as a 64-bit address it cost that kernel 2 to 3 spilled
    // VGPRs under its 128)
    unsigned off = (unsigned)X * 4u;
    asm volatile("" : "+v"(off));
    st_stream_quad_a8(outp + (size_t)((unsigned)i * g.lo.pitch), off,
                      make_uint4(y210_half(y[0], s0.x, g.nv.cbo), y210_half(y[1], s0.y, g.nv.cro),
                                 y210_half(y[2], s1.x, g.nv.cbo), y210_half(y[3], s1.y, g.nv.cro)));
}
// The fused kernels' (I, Q) of source columns X-1 .. X+4 (cl, cr: the outer two,
// wrapped or clamped) of source row `row`
__device__ __forceinline__ void y210_quad_iq(const uint8_t *img, const Geo &g, int row, unsigned X, unsigned cl,
                                             unsigned cr, c2 (&a)[6])
{
    const uint2 pl = ld_off<uint2>(img, y210_off(g, row, cl));
    const uint4 pm = ld_quad_a8(img, y210_off(g, row, X));
    const uint2 pr = ld_off<uint2>(img, y210_off(g, row, cr));
    a[0] = y210_iq2(pl, g);
    a[1] = a[2] = y210_iq2(make_uint2(pm.x, pm.y), g);
    a[3] = a[4] = y210_iq2(make_uint2(pm.z, pm.w), g);
    a[5] = y210_iq2(pr, g);
}

// =========================================================================
// K1: luma rows -> half spectra of row pairs
// =========================================================================
// GEN (odd W or H): the composite taps of a pixel span i-2 .. i+1 and are
// read as unmerged Tap4 entries (colT / rowT) instead of the 3-tap tables.
template <int LOG2N, int FMT, bool GEN = false, bool LAT = false>
__global__ __launch_bounds__((k1_gpw<LOG2N, LAT>() * fft_T<LOG2N>()))
void k_rows_fwd(const uint8_t *__restrict__ frames, int pairs_per_frame,
                int total_pairs, Geo g, const float4 *__restrict__ colW3,
                const float4 *__restrict__ rowW3, const Tap4 *__restrict__ colT,
                const Tap4 *__restrict__ rowT, const c2 *__restrict__ tw,
                c2 *__restrict__ G, size_t g_stride)
{
    constexpr int N = 1 << LOG2N, T = fft_T<LOG2N>(), GPW = k1_gpw<LOG2N, LAT>();
    extern __shared__ __attribute__((aligned(16))) c2 lds_all[];
    // group index: wave-uniform (scalar) when a group spans whole waves
    const int grp = GPW == 1 ? 0 : (T % 64 == 0 ? __builtin_amdgcn_readfirstlane(threadIdx.x / T)
                                               : threadIdx.x / T);
    const int t = GPW == 1 ? threadIdx.x : threadIdx.x % T;
    c2 *lds = lds_all + grp * lds_complex<N>();
    const int lblk = xcd_remap(blockIdx.x, gridDim.x) * GPW;   // block's first pair
    const int logical = lblk + grp;
    const bool valid = logical < total_pairs;
    const int frame = valid ? logical / pairs_per_frame : 0;
    const int ra = valid ? 2 * (logical % pairs_per_frame) : 0;  // image row of pair
    const uint8_t *img = frames + (size_t)frame * g.li.stride;

    // vertical part of the separable resample: V_a, V_b over all source columns.
    // Taps of image row r lie on source rows r-1..r+1 (w3 tables), so the pair
    // (ra, ra+1) reads the 4 source rows ra-1..ra+2.
    float *V = reinterpret_cast<float *>(lds);   // GEN: [2][W] (rows a, b)
    c2 *V2 = lds;                                 // 3-tap path: [W] (row a, row b) pairs
    using raw_t = typename LumaSrc<FMT>::raw_t;
    constexpr int BPP = LumaSrc<FMT>::bpp;
    const float lu = k1_unit<FMT>(g);   // a constant but for NV12 (its range's 1/219 or 1/255)
    // one-pair workgroups (LAT: short launches, latency-bound) issue the
    // column taps and twiddles with the pixel loads instead of one dependent
    // round trip each after them (batch launches: K1 +5 %, registers held
    // across the loads)
    c2 wb[kTwSlots];
    float4 cw[8];
    if constexpr (LAT && !GEN) {
        preload_twiddles_wl<LOG2N>(wb, t, tw);
#pragma unroll
        for (int j = 0; j < 8; ++j) cw[j] = colW3[min(max(t + j * T - g.x0, 0), g.W - 1)];
    }
    // RGBA8 / RGBA16F: all 32 pixel loads of the thread in one batch; RGBA32F
    // (4x the registers of RGBA8): two batches of 16
    // (MM_Y210's matrixed instance, 8-byte loads, at N = 8192, where 1024
    // threads leave 128 VGPRs: two batches too; one batch spilled 21; the
    // matrixed three-plane instance, two chroma byte loads per pair, the same:
    // one batch spilled 29; its 10-bit form, two chroma word loads per pair:
    // one batch spilled 27)
    // (v210's matrixed instance, the same 8 bytes per tap as MM_Y210's plus the
    // field positions of each column: four batches of two there; two batches
    // spilled 10 in the one-pair form.  DESIGN.md "v210 capture frames" has the
    // register table)
    constexpr int UB = FMT == kFmtV210M && LOG2N == 13 ? 2
                       : BPP == 16 || ((FMT == kFmtY210M || FMT == kFmtI420M || FMT == kFmtI010M) && LOG2N == 13) ? 4 : 8;
    if constexpr (GEN) {
        if (valid) {
            Tap4 ta = rowT[ra];
            Tap4 tb = ra + 1 < g.H ? rowT[ra + 1] : ta;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                ta.w[m] *= lu;
                tb.w[m] = ra + 1 < g.H ? tb.w[m] * lu : 0.0f;   // the zero row of odd H
            }
            unsigned pa[4], pb[4];   // source row byte offsets
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                pa[m] = (unsigned)wrap_near(ta.idx[m], g.H, g.edge) * g.li.pitch;
                pb[m] = (unsigned)wrap_near(tb.idx[m], g.H, g.edge) * g.li.pitch;
            }
            for (int i = t; i < g.W; i += T) {
                float va = 0.0f, vb = 0.0f;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    if constexpr (kRGB24<FMT>) {   // (the byte-aligned dword of pixel i)
                        va += ta.w[m] * rgb24_luma_units(rgb24_px(img, pa[m], (unsigned)i, g), g);
                        vb += tb.w[m] * rgb24_luma_units(rgb24_px(img, pb[m], (unsigned)i, g), g);
                    } else {
                        va += ta.w[m] * k1_luma<FMT>(ld_off<raw_t>(img, pa[m] + (unsigned)i * BPP), g);
                        vb += tb.w[m] * k1_luma<FMT>(ld_off<raw_t>(img, pb[m] + (unsigned)i * BPP), g);
                    }
                }
                V[i] = va;
                V[g.W + i] = vb;
            }
        }
    } else if (GPW == 2 && !LAT && pairs_per_frame % 2 == 0) {
        // Batch form, the two groups' row pairs in one frame (uniform test):
        // the workgroup's 4 rows r0 .. r0+3 read the 6 source rows r0-1 ..
        // r0+4 once, shared (each group alone read 4: 8 row loads for 4
        // rows); thread tid of the 2T does N/(2T) columns for both groups.
        // Same lumas and the same packed expressions per group as below: the
        // V2 values are bitwise the per-group form's.
        if (valid) {
            const int r0 = ra - 2 * grp;   // group 0's pair (same frame: pairs_per_frame even)
            c2 w[2][3];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                float4 wa = rowW3[r0 + 2 * q], wb = rowW3[r0 + 2 * q + 1];
                wa.x *= lu, wa.y *= lu, wa.z *= lu;
                wb.x *= lu, wb.y *= lu, wb.z *= lu;
                w[q][0] = mk(wa.x, wb.x);
                w[q][1] = mk(wa.y, wb.y);
                w[q][2] = mk(wa.z, wb.z);
            }
            const uint8_t *rowp[6];   // workgroup-uniform source row pointers
#pragma unroll
            for (int d = 0; d < 6; ++d) rowp[d] = img + (unsigned)wrap_near(r0 - 1 + d, g.H, g.edge) * g.li.pitch;
            // matrixed 4:2:0: the 6 source rows lie on 4 chroma rows (r0 is
            // even: rows r0, r0+1 and r0+2, r0+3 share one each), loaded once
            // per column in the same batch as the lumas
            [[maybe_unused]] const uint8_t *crowp[4];
            if constexpr (kMatrixed<FMT>) {
                crowp[0] = k1_crow<FMT>(img, g, wrap_near(r0 - 1, g.H, g.edge));
                crowp[1] = k1_crow<FMT>(img, g, r0);
                crowp[2] = k1_crow<FMT>(img, g, r0 + 2);
                crowp[3] = k1_crow<FMT>(img, g, wrap_near(r0 + 4, g.H, g.edge));
            }
            constexpr int CT = N / (2 * T);          // columns per thread (W <= N)
            constexpr int CB = BPP == 16 ? 1 : CT;   // columns per load batch
            c2 *V2g1 = lds_all + lds_complex<N>();
#pragma unroll
            for (int h = 0; h < CT / CB; ++h) {
                __builtin_amdgcn_sched_barrier(0);
                raw_t px[CB][6];
                [[maybe_unused]] typename ChromaSrc<FMT>::raw_t cx[CB][4];
#pragma unroll
                for (int u = 0; u < CB; ++u) {
                    const unsigned col = (unsigned)min((int)threadIdx.x + (h * CB + u) * 2 * T, g.W - 1);
                    const unsigned off = k1_off<FMT>(col, g);
#pragma unroll
                    for (int d = 0; d < 6; ++d) px[u][d] = k1_ld<FMT>(rowp[d], off);
                    if constexpr (kMatrixed<FMT>) {
#pragma unroll
                        for (int d = 0; d < 4; ++d)
                            cx[u][d] = k1_cld<FMT>(crowp[d], col, g);
                    }
                }
#pragma unroll
                for (int u = 0; u < CB; ++u) {
                    const int i = (int)threadIdx.x + (h * CB + u) * 2 * T;
                    float l[6];
#pragma unroll
                    for (int d = 0; d < 6; ++d) l[d] = k1_luma_at<FMT>(px[u][d], (unsigned)min(i, g.W - 1), g);
                    if constexpr (kMatrixed<FMT>) {
#pragma unroll
                        for (int d = 0; d < 6; ++d) l[d] += k1_chroma<FMT>(cx[u][(d + 1) >> 1], g);
                    }
                    if (i < g.W) {
                        lds_all[i] = w[0][0] * mk(l[0], l[1]) + w[0][1] * mk(l[1], l[2]) + w[0][2] * mk(l[2], l[3]);
                        V2g1[i] = w[1][0] * mk(l[2], l[3]) + w[1][1] * mk(l[3], l[4]) + w[1][2] * mk(l[4], l[5]);
                    }
                }
            }
        }
    } else if (valid) {
        // odd H: the last pair's second row is outside the image (zero)
        float4 wa = rowW3[ra], wb = ra + 1 < g.H ? rowW3[ra + 1] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        wa.x *= lu, wa.y *= lu, wa.z *= lu;
        wb.x *= lu, wb.y *= lu, wb.z *= lu;
        // rows a and b as one packed pair: (a, b) = (wa.x, wb.x) (l0, l1) +
        // (wa.y, wb.y) (l1, l2) + (wa.z, wb.z) (l2, l3), per lane the scalar
        // forms' fma chains (half the VALU instructions, one 8-B LDS store)
        const c2 w0 = mk(wa.x, wb.x), w1 = mk(wa.y, wb.y), w2 = mk(wa.z, wb.z);
        const uint8_t *rowp[4];   // workgroup-uniform source row pointers
#pragma unroll
        for (int d = 0; d < 4; ++d) rowp[d] = img + (unsigned)wrap_near(ra - 1 + d, g.H, g.edge) * g.li.pitch;
        // matrixed 4:2:0 (H even, so ra + 1 < H): the 4 source rows lie on 3
        // chroma rows (ra and ra + 1 share one), loaded once per column in the
        // same batch as the lumas
        [[maybe_unused]] const uint8_t *crowp[3];
        if constexpr (kMatrixed<FMT>) {
            crowp[0] = k1_crow<FMT>(img, g, wrap_near(ra - 1, g.H, g.edge));
            crowp[1] = k1_crow<FMT>(img, g, ra);
            crowp[2] = k1_crow<FMT>(img, g, wrap_near(ra + 2, g.H, g.edge));
        }
        // W <= N = 8T: at most 8 columns per thread
#pragma unroll
        for (int h = 0; h < 8 / UB; ++h) {
            __builtin_amdgcn_sched_barrier(0);
            raw_t px[UB][4];
            [[maybe_unused]] typename ChromaSrc<FMT>::raw_t cx[UB][3];
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const unsigned col = (unsigned)min(t + (h * UB + u) * T, g.W - 1);
                const unsigned off = k1_off<FMT>(col, g);
#pragma unroll
                for (int d = 0; d < 4; ++d) px[u][d] = k1_ld<FMT>(rowp[d], off);
                if constexpr (kMatrixed<FMT>) {
#pragma unroll
                    for (int d = 0; d < 3; ++d)
                        cx[u][d] = k1_cld<FMT>(crowp[d], col, g);
                }
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int i = t + (h * UB + u) * T;
                float l[4];
#pragma unroll
                for (int d = 0; d < 4; ++d) l[d] = k1_luma_at<FMT>(px[u][d], (unsigned)min(i, g.W - 1), g);
                if constexpr (kMatrixed<FMT>) {
#pragma unroll
                    for (int d = 0; d < 4; ++d) l[d] += k1_chroma<FMT>(cx[u][(d + 1) >> 1], g);
                }
                if (i < g.W) V2[i] = w0 * mk(l[0], l[1]) + w1 * mk(l[1], l[2]) + w2 * mk(l[2], l[3]);
            }
        }
    }
    __syncthreads();
    // all 8 colW3 loads in one batch (two batches of 4: one more dependent
    // L2 round trip per pair, K1 +5 %)
    c2 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int i = t + j * T - g.x0;                    // image column
        const int ic = min(max(i, 0), g.W - 1);
        float ya = 0.0f, yb = 0.0f;
        if constexpr (GEN) {
            const Tap4 tc = colT[ic];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int c = wrap_near(tc.idx[m], g.W, g.edge);
                ya += tc.w[m] * V[c];
                yb += tc.w[m] * V[g.W + c];
            }
        } else {
            const float4 w = LAT ? cw[j] : colW3[ic];   // weights of source columns i-1, i, i+1; .w: wrapped
            const unsigned nb = __float_as_uint(w.w);          // (i-1) | (i+1) << 16
            const int cl = nb & 0xffffu, cr = nb >> 16;
            const c2 y2 = w.x * V2[cl] + w.y * V2[ic] + w.z * V2[cr];   // (ya, yb)
            ya = y2.x;
            yb = y2.y;
        }
        const bool in = valid && i >= 0 && i < g.W;
        v[j] = in ? mk(ya, yb) : mk(0.0f, 0.0f);
    }
    if constexpr (!LAT || GEN) preload_twiddles_wl<LOG2N>(wb, t, tw);
    __syncthreads();
    fft_dif<LOG2N, -1>(v, t, lds, wb);
    __syncthreads();   // every wave done with its LDS region
#pragma unroll
    for (int j = 0; j < 8; ++j) lds[zslot<LOG2N>(fft_bin<LOG2N>(t, j))] = v[j];
    __syncthreads();
    // half spectra of rows (ra, ra+1) at bins f = t + jT (j < 4) and N/2 (j = 4)
    auto split = [&](int f) {
        c2 zf = lds[zslot<LOG2N>(f)], zm = lds[zslot<LOG2N>((N - f) & (N - 1))];
        // Y_a = (Z[f] + conj Z[N-f]) / 2 ;  Y_b = (Z[f] - conj Z[N-f]) / 2i
        float4 o;
        o.x = 0.5f * (zf.x + zm.x);
        o.y = 0.5f * (zf.y - zm.y);
        o.z = 0.5f * (zf.y + zm.y);
        o.w = -0.5f * (zf.x - zm.x);
        return o;
    };
    float4 o[5];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = split(t + j * T);
    o[4] = split(N / 2);
    // G[f][row] is row-contiguous per bin.  With whole row-pair groups per
    // frame in the workgroup (uniform test), the GPW pairs' values of a bin are
    // transposed through LDS and leave as one 16*GPW-byte piece (consecutive
    // rows); else every group stores its own 16-B pieces.
    if (GPW == 1 || pairs_per_frame % GPW != 0) {
        if (!valid) return;
        c2 *Gf = G + (size_t)frame * g_stride;
#pragma unroll
        for (int j = 0; j < 4; ++j) st_off<float4>(Gf, (unsigned)((t + j * T) * g.Hg + ra) * 8u, o[j]);
        if (t == 0) st_off<float4>(Gf, (unsigned)((N / 2) * g.Hg + ra) * 8u, o[4]);
        return;
    }
    __syncthreads();   // split reads done before the staging overwrites the buffers
    // [GPW][SS] (group-major, SS = N/2+1 rounded up to 8 mod 16 float4: the two
    // groups' entries of a bin 32 banks apart) when GPW == 2; [N/2 + 1][GPW]
    // otherwise (small N: many groups, no room for padding)
    float4 *stg = reinterpret_cast<float4 *>(lds_all);
    constexpr int SS = (N / 2 + 1 + 7) / 16 * 16 + 8;
    constexpr bool GM = GPW == 2 && 2 * SS * 2 <= 2 * lds_complex<N>();
    auto sidx = [&](int f, int c) { return GM ? c * SS + f : f * GPW + c; };
#pragma unroll
    for (int j = 0; j < 4; ++j) stg[sidx(t + j * T, grp)] = o[j];
    if (t == 0) stg[sidx(N / 2, grp)] = o[4];
    __syncthreads();
    if (lblk >= total_pairs) return;   // whole block past the end (total % GPW == 0)
    const int fr0 = lblk / pairs_per_frame, ra0 = 2 * (lblk % pairs_per_frame);
    c2 *Gf = G + (size_t)fr0 * g_stride;
    for (int e = threadIdx.x; e < (N / 2 + 1) * GPW; e += GPW * T) {
        const int f = e / GPW, c = e - f * GPW;
        st_off<float4>(Gf, (unsigned)(f * g.Hg + ra0 + 2 * c) * 8u, stg[sidx(f, c)]);
    }
}

// =========================================================================
// K2: column FFT -> pyramid phase magnification -> column IFFT
// =========================================================================
__device__ __forceinline__ float smooth01(float x)   // HLSL smoothstep(0,1,x)
{
    float t = sat(x);
    return t * t * (3.0f - 2.0f * t);
}

// atan2 for the phase difference: octant reduction + degree-15 odd minimax
// polynomial on [0,1] (|err| <= 1.5e-7 rad; the phase scale S multiplies it).
__device__ __forceinline__ float fast_atan2(float y, float x)
{
    const float ax = fabsf(x), ay = fabsf(y);
    // max3 with the smallest normal float: atan2(0, 0) = 0 without a select
    // (0 * rcp(2^-126) = 0); no nonzero argument of the ops is that small
    // (mn by the octant compare, not fminf: its NaN canonicalisation costs two
    // more instructions on operands the compiler cannot prove canonical)
    const bool steep = ay > ax;
    const float mx = fmaxf(fmaxf(ax, ay), 1.17549435e-38f), mn = steep ? ax : ay;
    const float a = mn * __builtin_amdgcn_rcpf(mx);
    const float s = a * a;
    float r = -0.00405455008149147f;
    r = r * s + 0.021862903609871864f;
    r = r * s - 0.055912263691425323f;
    r = r * s + 0.09642193466424942f;
    r = r * s - 0.1390862911939621f;
    r = r * s + 0.19946566224098206f;
    r = r * s - 0.33329859375953674f;
    r = r * s + 0.9999993443489075f;
    r *= a;
    if (steep) r = 1.57079632679489662f - r;
    if (x < 0.0f) r = 3.14159265358979324f - r;
    return copysignf(r, y);
}

// fast_atan2 of two arguments at once: the polynomial, its reconstruction
// constant and the scale run as packed FP32 (v_pk_fma_f32: a fused
// multiply-add per half, so both results are fast_atan2's bit for bit); the
// octant selects stay scalar (VOP3P has no abs modifier)
__device__ __forceinline__ c2 fast_atan2_x2(float y0, float x0, float y1, float x1)
{
    const float ax0 = fabsf(x0), ay0 = fabsf(y0), ax1 = fabsf(x1), ay1 = fabsf(y1);
    const bool st0 = ay0 > ax0, st1 = ay1 > ax1;
    const float a0 = (st0 ? ax0 : ay0) * __builtin_amdgcn_rcpf(fmaxf(fmaxf(ax0, ay0), 1.17549435e-38f));
    const float a1 = (st1 ? ax1 : ay1) * __builtin_amdgcn_rcpf(fmaxf(fmaxf(ax1, ay1), 1.17549435e-38f));
    const c2 a = mk(a0, a1), sq = a * a;
    c2 r = mk(-0.00405455008149147f, -0.00405455008149147f);
    r = r * sq + mk(0.021862903609871864f, 0.021862903609871864f);
    r = r * sq - mk(0.055912263691425323f, 0.055912263691425323f);
    r = r * sq + mk(0.09642193466424942f, 0.09642193466424942f);
    r = r * sq - mk(0.1390862911939621f, 0.1390862911939621f);
    r = r * sq + mk(0.19946566224098206f, 0.19946566224098206f);
    r = r * sq - mk(0.33329859375953674f, 0.33329859375953674f);
    r = r * sq + mk(0.9999993443489075f, 0.9999993443489075f);
    const c2 ra = r * a;
    const c2 rs = mk(1.57079632679489662f, 1.57079632679489662f) - ra;
    float t0 = st0 ? rs.x : ra.x, t1 = st1 ? rs.y : ra.y;
    if (x0 < 0.0f) t0 = 3.14159265358979324f - t0;
    if (x1 < 0.0f) t1 = 3.14159265358979324f - t1;
    return mk(copysignf(t0, y0), copysignf(t1, y1));
}

// Radial masks of GeneratePyramidFilters (PyramidOperations.compute:25-87) and the
// per-level gate/phase rule of ProcessPyramidPhaseDifference
// (PyramidPhaseDifference.compute:58-101), summed over levels
// (AccumulatePyramidLevel, PyramidOperations.compute:111-128), for one bin:
//   A = c * [ sum_{pass} m_i + sum_{mag} m_i * e^{i S wrap(arg p - arg c)} ] / N^2
// Levels 0 and L-1 always pass; a middle level passes where |m c| or |m p| < tau.
template <int LOG2N>
__device__ __forceinline__ c2 pyramid_op(c2 c, c2 p, int fx, int fy, const Spec &sp)
{
    constexpr int N = 1 << LOG2N;
    const float ux = (float)fx * (1.0f / (float)N);
    const float uy = (float)(fy <= N / 2 ? fy : N - fy) * (1.0f / (float)N);
    const float fr = __builtin_amdgcn_sqrtf(ux * ux + uy * uy);
    const float mn2 = fminf(c.x * c.x + c.y * c.y, p.x * p.x + p.y * p.y);
    // level 0: high-pass
    float mpass = fr > sp.maxF ? 1.0f : (fr > sp.hp_lo ? smooth01((fr - sp.hp_lo) * sp.hp_inv) : 0.0f);
    // level L-1: low-pass
    if (sp.L > 1)
        mpass += fr < sp.minF ? 1.0f : (fr < sp.lp_hi ? 1.0f - smooth01((fr - sp.minF) * sp.lp_inv) : 0.0f);
    float mmag = 0.0f;
    for (int i = 1; i < sp.L - 1; ++i) {
        if (fr >= sp.lo[i] && fr <= sp.hi[i]) {
            const float m = 0.5f * (1.0f + __cosf(2.0f * kPi * ((fr - sp.lo[i]) * sp.inv_w[i] - 0.5f)));
            if (m * m * mn2 < sp.tau2) mpass += m;
            else mmag += m;
        }
    }
    c2 a = scale(c, mpass * sp.inv_nn);
    if (mmag > 0.0f) {
        // delta = wrap(arg p - arg c) = arg(p * conj c); an exactly zero p
        // (ungated only at tau = 0: a black previous frame) has arg p =
        // atan2(0, 0) = 0 in the reference, so delta = -arg c = arg(conj c)
        const bool pz = p.x == 0.0f && p.y == 0.0f;
        const float d = fast_atan2(pz ? -c.y : p.y * c.x - p.x * c.y, pz ? c.x : p.x * c.x + p.y * c.y);
        const float ph = sp.S * d;
        const float k = mmag * sp.inv_nn;
        a = add(a, scale(mul_c(c, mk(__cosf(ph), __sinf(ph))), k));
    }
    return a;
}

// ProcessPhaseDifference (PhaseDifferenceComputeShader.compute:124-179) for one
// bin of the unmasked spectrum (standard mode, .cs:208-232):
//   A = c * e^{i S w(sf) wrap(arg p - arg c)} / N^2, or c / N^2 if |c| or |p| < tau,
// w = calculate_bandpass_weight(calculate_spatial_frequency) (:74-122).
template <int LOG2N>
__device__ __forceinline__ c2 standard_op(c2 c, c2 p, int fx, int fy, const Spec &sp)
{
    constexpr int N = 1 << LOG2N;
    const float ux = (float)fx * (1.0f / (float)N);
    const float uy = (float)(fy <= N / 2 ? fy : N - fy) * (1.0f / (float)N);
    const float sf = fminf(__builtin_amdgcn_sqrtf(ux * ux + uy * uy) / 0.707f, 1.0f);
    const float mn2 = fminf(c.x * c.x + c.y * c.y, p.x * p.x + p.y * p.y);
    if (mn2 < sp.tau2) return scale(c, sp.inv_nn);
    float w = 1.0f;
    if (sp.bp_apply) {
        if (sf < sp.bp_low) w *= __powf(sf * sp.bp_inv_low, sp.bp_steep);
        if (sf > sp.bp_high) w *= __powf((1.0f - sf) * sp.bp_inv_1mhigh, sp.bp_steep);
        w *= sp.bp_sens;
        if (sf > sp.bp_low && sf < sp.bp_high)
            w *= 1.0f + sp.bp_edge * __sinf(kPi * (sf - sp.bp_low) * sp.bp_inv_band);
        w = fmaxf(w, 0.0f);
    }
    const float d = fast_atan2(p.y * c.x - p.x * c.y, p.x * c.x + p.y * c.y);
    const float ph = (d * w) * sp.S;
    return scale(mul_c(c, mk(__cosf(ph), __sinf(ph))), sp.inv_nn);
}

template <int LOG2N, int MODE>
__device__ __forceinline__ c2 spectral_op(c2 c, c2 p, int fx, int fy, const Spec &sp)
{
    if constexpr (MODE == 0) return pyramid_op<LOG2N>(c, p, fx, fy, sp);
    else return standard_op<LOG2N>(c, p, fx, fy, sp);
}

// ---- frame-invariant part of the spectral op: per-bin LDS table ---------
// A thread owns the same bins of one column for every frame of a launch, so
// what depends only on (fx, fy) is evaluated once per launch into LDS (N/2+1
// entries: every mask is symmetric in fy) instead of once per bin and frame.
//   MM_K2_PYR_TAB (pyramid): x = m_a, the first middle-band mask nonzero at
//     the bin; y = -(m_a + hp + lp), minus the bin's mask sum (hp, lp: the
//     always-passed levels 0 and L-1), when at most one band is nonzero (sign
//     bit set, -0.0 included), else y = m_b, the second band, and hp + lp is
//     evaluated inline (a divergent branch that only waves holding such bins
//     take; none for L <= 5 at default bands).
//     The host checks that no 3 bands overlap.
//   MM_MODE_STANDARD: (w, 0), w = calculate_bandpass_weight (:74-122).
constexpr int MM_K2_PYR_TAB = 2;
// MM_K2_PYR_TAB2: MM_K2_PYR_TAB for band layouts whose neighbouring middle
// bands overlap (L = 6 at the default 0.05 / 0.45: the C3 configuration).
// Waves holding a two-band bin run pyramid_op_2band_x2 (branch-free, the
// bins' whole mask sums from a second LDS array) instead of the generic
// one-bin-at-a-time op; the table is MM_K2_PYR_TAB's.  A separate kernel
// instance, so that the one-band layouts' kernel keeps its registers.
constexpr int MM_K2_PYR_TAB2 = 4;
template <int MODE> constexpr bool k2_tabled()
{
    return MODE == MM_K2_PYR_TAB || MODE == MM_K2_PYR_TAB2;
}
template <int MODE> constexpr bool k2_msum() { return MODE == MM_K2_PYR_TAB2; }
template <int MODE> constexpr bool k2_one_band_op() { return MODE == MM_K2_PYR_TAB || MODE == MM_K2_PYR_TAB2; }

template <int LOG2N, int MODE>
__device__ __forceinline__ float2 bin_static(int fx, int fyy, const Spec &sp)
{
    constexpr int N = 1 << LOG2N;
    const float ux = (float)fx * (1.0f / (float)N);
    const float uy = (float)fyy * (1.0f / (float)N);
    const float fr = __builtin_amdgcn_sqrtf(ux * ux + uy * uy);
    if constexpr (MODE == MM_MODE_STANDARD) {
        const float sf = fminf(fr / 0.707f, 1.0f);
        float w = 1.0f;
        if (sp.bp_apply) {
            if (sf < sp.bp_low) w *= __powf(sf * sp.bp_inv_low, sp.bp_steep);
            if (sf > sp.bp_high) w *= __powf((1.0f - sf) * sp.bp_inv_1mhigh, sp.bp_steep);
            w *= sp.bp_sens;
            if (sf > sp.bp_low && sf < sp.bp_high)
                w *= 1.0f + sp.bp_edge * __sinf(kPi * (sf - sp.bp_low) * sp.bp_inv_band);
            w = fmaxf(w, 0.0f);
        }
        return make_float2(w, 0.0f);
    } else {
        float mfix = fr > sp.maxF ? 1.0f : (fr > sp.hp_lo ? smooth01((fr - sp.hp_lo) * sp.hp_inv) : 0.0f);
        if (sp.L > 1)
            mfix += fr < sp.minF ? 1.0f : (fr < sp.lp_hi ? 1.0f - smooth01((fr - sp.minF) * sp.lp_inv) : 0.0f);
        float ma = 0.0f, mb = 0.0f;
        for (int i = 1; i < sp.L - 1; ++i) {
            if (fr >= sp.lo[i] && fr <= sp.hi[i]) {
                const float m = 0.5f * (1.0f + __cosf(2.0f * kPi * ((fr - sp.lo[i]) * sp.inv_w[i] - 0.5f)));
                if (m != 0.0f) {
                    if (ma == 0.0f) ma = m;
                    else mb = m;
                }
            }
        }
        // one band: y = -(m_a + hp + lp), the bin's whole mask sum (sign bit set,
        // -0.0 included); two bands: y = m_b > 0
        return make_float2(ma, mb != 0.0f ? mb : -(ma + mfix));
    }
}

// The bin's whole mask sum (every level, the K2 tables' second array): the
// pass weight of the two-band op.  For a one-band bin it is -y of
// bin_static's entry bit for bit (the same sum, ma + hp + lp).
template <int LOG2N>
__device__ __forceinline__ float bin_mask_sum(int fx, int fyy, const Spec &sp)
{
    constexpr int N = 1 << LOG2N;
    const float ux = (float)fx * (1.0f / (float)N);
    const float uy = (float)fyy * (1.0f / (float)N);
    const float fr = __builtin_amdgcn_sqrtf(ux * ux + uy * uy);
    float mfix = fr > sp.maxF ? 1.0f : (fr > sp.hp_lo ? smooth01((fr - sp.hp_lo) * sp.hp_inv) : 0.0f);
    if (sp.L > 1)
        mfix += fr < sp.minF ? 1.0f : (fr < sp.lp_hi ? 1.0f - smooth01((fr - sp.minF) * sp.lp_inv) : 0.0f);
    float ma = 0.0f, mb = 0.0f;
    for (int i = 1; i < sp.L - 1; ++i) {
        if (fr >= sp.lo[i] && fr <= sp.hi[i]) {
            const float m = 0.5f * (1.0f + __cosf(2.0f * kPi * ((fr - sp.lo[i]) * sp.inv_w[i] - 0.5f)));
            if (m != 0.0f) {
                if (ma == 0.0f) ma = m;
                else mb = m;
            }
        }
    }
    return mb != 0.0f ? (ma + mb) + mfix : ma + mfix;
}

// atan2 for a nonzero argument (the magnified bins: |u| = |p||c| > 0 there)
__device__ __forceinline__ float atan2_nz(float y, float x)
{
    const float ax = fabsf(x), ay = fabsf(y);
    // (the max3 guard of fast_atan2: atan2(0, 0) = 0, not 0 * rcp(0) = NaN, should
    // a zero bin get here ungated)
    const float a = fminf(ax, ay) * __builtin_amdgcn_rcpf(fmaxf(fmaxf(ax, ay), 1.17549435e-38f));
    const float s = a * a;
    float r = -0.00405455008149147f;
    r = r * s + 0.021862903609871864f;
    r = r * s - 0.055912263691425323f;
    r = r * s + 0.09642193466424942f;
    r = r * s - 0.1390862911939621f;
    r = r * s + 0.19946566224098206f;
    r = r * s - 0.33329859375953674f;
    r = r * s + 0.9999993443489075f;
    r *= a;
    if (ay > ax) r = 1.57079632679489662f - r;
    if (x < 0.0f) r = 3.14159265358979324f - r;
    return copysignf(r, y);
}

// pyramid_op with the middle bands from the table.  Table entries are the
// masks times inv_nn = 1/N^2 (a power of two, so every product and sum below
// is the unscaled one times inv_nn exactly, and the gate m^2 mn2 < tau^2 reads
// (m inv_nn)^2 mn2 < tau^2 inv_nn^2 with the same outcome):
//   A = c * [mpass + mmag e^{i S delta}],  delta = arg(p conj c)
template <int LOG2N>
__device__ __forceinline__ c2 pyramid_op_t(c2 c, c2 p, int fx, int fy, const Spec &sp, float2 mt)
{
    constexpr int N = 1 << LOG2N;
    const float mn2 = fminf(c.x * c.x + c.y * c.y, p.x * p.x + p.y * p.y);
    float mpass, mb;
    if (__builtin_signbit(mt.y)) {   // static hp + lp from the table
        mpass = -mt.y - mt.x;
        mb = 0.0f;
    } else {                         // two bands at this bin: hp + lp inline
        const float ux = (float)fx * (1.0f / (float)N);
        const float uy = (float)(fy <= N / 2 ? fy : N - fy) * (1.0f / (float)N);
        const float fr = __builtin_amdgcn_sqrtf(ux * ux + uy * uy);
        mpass = fr > sp.maxF ? 1.0f : (fr > sp.hp_lo ? smooth01((fr - sp.hp_lo) * sp.hp_inv) : 0.0f);
        if (sp.L > 1)
            mpass += fr < sp.minF ? 1.0f : (fr < sp.lp_hi ? 1.0f - smooth01((fr - sp.minF) * sp.lp_inv) : 0.0f);
        mpass *= sp.inv_nn;
        mb = mt.y;
    }
    float mmag = 0.0f;
    if (mt.x * mt.x * mn2 < sp.tau2_nn) mpass += mt.x;
    else mmag += mt.x;
    if (mb * mb * mn2 < sp.tau2_nn) mpass += mb;
    else mmag += mb;
    c2 w = mk(mpass, 0.0f);
    if (mmag > 0.0f) {
        // S * delta in revolutions straight into v_sin / v_cos
        const float rev = atan2_nz(p.y * c.x - p.x * c.y, p.x * c.x + p.y * c.y) * sp.S_rev;
        w = mk(mmag * __builtin_amdgcn_cosf(rev) + mpass, mmag * __builtin_amdgcn_sinf(rev));
    }
    return mul_c(c, w);
}

// pyramid_op_t for a bin with at most one middle band (table entry y < 0,
// the usual case: bands touch only where their masks are 0), without
// branches or selects on the phase factor, so that the compiler interleaves
// several bins' dependency chains (atan2 polynomial, v_sin/v_cos) instead of
// branching around each one under an exec mask:
//   w = mpass + mmag e^{i S delta},  mmag = gated ? 0 : m_a,  mpass = sum - mmag
// (mmag = 0 gives w = (mpass, 0) exactly: cos/sin are finite for every
// argument, fast_atan2(0, 0) = 0).  u = p conj c and c w use the packed
// multiplies (their operands are plain VALU results, never a transcendental's).
__device__ __forceinline__ c2 pyramid_op_1band(c2 c, c2 p, const Spec &sp, float2 mt)
{
    const float mn2 = fminf(c.x * c.x + c.y * c.y, p.x * p.x + p.y * p.y);
    const float mmag = mt.x * mt.x * mn2 < sp.tau2_nn ? 0.0f : mt.x;
    const float mpass = -mt.y - mmag;
    const c2 u = mul_conj(p, c);
    const float rev = fast_atan2(u.y, u.x) * sp.S_rev;
    const float cw = __builtin_amdgcn_cosf(rev), sw = __builtin_amdgcn_sinf(rev);
    return mul(c, mk(mmag * cw + mpass, mmag * sw));
}

// pyramid_op_1band for two bins at once: the same operations, with the
// atan2 polynomial, its reconstruction and the scale to revolutions of both
// bins in packed FP32 (one v_pk_fma per step for two bins; v_pk_fma_f32 is a
// fused multiply-add per half, so every value is the scalar form's bit for
// bit).  Only the per-bin octant selects stay scalar (no abs modifier on
// VOP3P sources).
__device__ __forceinline__ void pyramid_op_1band_x2(c2 &v0, c2 &p0, float2 mt0, c2 &v1, c2 &p1, float2 mt1,
                                                    const Spec &sp)
{
    const c2 c0 = v0, c1 = v1;
    const float mn0 = fminf(c0.x * c0.x + c0.y * c0.y, p0.x * p0.x + p0.y * p0.y);
    const float mn1 = fminf(c1.x * c1.x + c1.y * c1.y, p1.x * p1.x + p1.y * p1.y);
    const float mmag0 = mt0.x * mt0.x * mn0 < sp.tau2_nn ? 0.0f : mt0.x;
    const float mmag1 = mt1.x * mt1.x * mn1 < sp.tau2_nn ? 0.0f : mt1.x;
    const float mpass0 = -mt0.y - mmag0, mpass1 = -mt1.y - mmag1;
    const c2 u0 = mul_conj(p0, c0), u1 = mul_conj(p1, c1);
    // octant reduction per bin (fast_atan2's expressions)
    const float ax0 = fabsf(u0.x), ay0 = fabsf(u0.y), ax1 = fabsf(u1.x), ay1 = fabsf(u1.y);
    const bool st0 = ay0 > ax0, st1 = ay1 > ax1;
    const float a0 = (st0 ? ax0 : ay0) * __builtin_amdgcn_rcpf(fmaxf(fmaxf(ax0, ay0), 1.17549435e-38f));
    const float a1 = (st1 ? ax1 : ay1) * __builtin_amdgcn_rcpf(fmaxf(fmaxf(ax1, ay1), 1.17549435e-38f));
    const c2 a = mk(a0, a1), sq = a * a;
    c2 r = mk(-0.00405455008149147f, -0.00405455008149147f);
    r = r * sq + mk(0.021862903609871864f, 0.021862903609871864f);
    r = r * sq - mk(0.055912263691425323f, 0.055912263691425323f);
    r = r * sq + mk(0.09642193466424942f, 0.09642193466424942f);
    r = r * sq - mk(0.1390862911939621f, 0.1390862911939621f);
    r = r * sq + mk(0.19946566224098206f, 0.19946566224098206f);
    r = r * sq - mk(0.33329859375953674f, 0.33329859375953674f);
    r = r * sq + mk(0.9999993443489075f, 0.9999993443489075f);
    const c2 ra = r * a;
    const c2 rs = mk(1.57079632679489662f, 1.57079632679489662f) - ra;
    float t0 = st0 ? rs.x : ra.x, t1 = st1 ? rs.y : ra.y;
    if (u0.x < 0.0f) t0 = 3.14159265358979324f - t0;
    if (u1.x < 0.0f) t1 = 3.14159265358979324f - t1;
    const c2 rev = mk(copysignf(t0, u0.y), copysignf(t1, u1.y)) * mk(sp.S_rev, sp.S_rev);
    const float cw0 = __builtin_amdgcn_cosf(rev.x), sw0 = __builtin_amdgcn_sinf(rev.x);
    const float cw1 = __builtin_amdgcn_cosf(rev.y), sw1 = __builtin_amdgcn_sinf(rev.y);
    v0 = mul(c0, mk(mmag0 * cw0 + mpass0, mmag0 * sw0));
    v1 = mul(c1, mk(mmag1 * cw1 + mpass1, mmag1 * sw1));
    p0 = c0;
    p1 = c1;
}

// pyramid_op_1band_x2 for waves that hold a bin with TWO middle bands (the
// L = 6 layouts: neighbouring raised-cosine bands overlap), branch-free like
// the one-band op instead of the generic per-bin path: each band is gated on
// its own (PyramidPhaseDifference.compute:82-86 per level),
//   w = msum - mmag + mmag e^{i S delta},  mmag = [m_a not gated] m_a + [m_b not gated] m_b,
// msum = the bin's whole mask sum (table's second array).  A one-band bin
// (mt.y < 0) has m_b = 0, whose gate always holds: the one-band op's values
// bit for bit (msum == -mt.y).
__device__ __forceinline__ void pyramid_op_2band_x2(c2 &v0, c2 &p0, float2 mt0, float ms0, c2 &v1, c2 &p1,
                                                    float2 mt1, float ms1, const Spec &sp)
{
    const c2 c0 = v0, c1 = v1;
    const float mn0 = fminf(c0.x * c0.x + c0.y * c0.y, p0.x * p0.x + p0.y * p0.y);
    const float mn1 = fminf(c1.x * c1.x + c1.y * c1.y, p1.x * p1.x + p1.y * p1.y);
    const float mb0 = fmaxf(mt0.y, 0.0f), mb1 = fmaxf(mt1.y, 0.0f);
    const float mmag0 = (mt0.x * mt0.x * mn0 < sp.tau2_nn ? 0.0f : mt0.x) + (mb0 * mb0 * mn0 < sp.tau2_nn ? 0.0f : mb0);
    const float mmag1 = (mt1.x * mt1.x * mn1 < sp.tau2_nn ? 0.0f : mt1.x) + (mb1 * mb1 * mn1 < sp.tau2_nn ? 0.0f : mb1);
    const float mpass0 = ms0 - mmag0, mpass1 = ms1 - mmag1;
    const c2 u0 = mul_conj(p0, c0), u1 = mul_conj(p1, c1);
    const float ax0 = fabsf(u0.x), ay0 = fabsf(u0.y), ax1 = fabsf(u1.x), ay1 = fabsf(u1.y);
    const bool st0 = ay0 > ax0, st1 = ay1 > ax1;
    const float a0 = (st0 ? ax0 : ay0) * __builtin_amdgcn_rcpf(fmaxf(fmaxf(ax0, ay0), 1.17549435e-38f));
    const float a1 = (st1 ? ax1 : ay1) * __builtin_amdgcn_rcpf(fmaxf(fmaxf(ax1, ay1), 1.17549435e-38f));
    const c2 a = mk(a0, a1), sq = a * a;
    c2 r = mk(-0.00405455008149147f, -0.00405455008149147f);
    r = r * sq + mk(0.021862903609871864f, 0.021862903609871864f);
    r = r * sq - mk(0.055912263691425323f, 0.055912263691425323f);
    r = r * sq + mk(0.09642193466424942f, 0.09642193466424942f);
    r = r * sq - mk(0.1390862911939621f, 0.1390862911939621f);
    r = r * sq + mk(0.19946566224098206f, 0.19946566224098206f);
    r = r * sq - mk(0.33329859375953674f, 0.33329859375953674f);
    r = r * sq + mk(0.9999993443489075f, 0.9999993443489075f);
    const c2 ra = r * a;
    const c2 rs = mk(1.57079632679489662f, 1.57079632679489662f) - ra;
    float t0 = st0 ? rs.x : ra.x, t1 = st1 ? rs.y : ra.y;
    if (u0.x < 0.0f) t0 = 3.14159265358979324f - t0;
    if (u1.x < 0.0f) t1 = 3.14159265358979324f - t1;
    const c2 rev = mk(copysignf(t0, u0.y), copysignf(t1, u1.y)) * mk(sp.S_rev, sp.S_rev);
    const float cw0 = __builtin_amdgcn_cosf(rev.x), sw0 = __builtin_amdgcn_sinf(rev.x);
    const float cw1 = __builtin_amdgcn_cosf(rev.y), sw1 = __builtin_amdgcn_sinf(rev.y);
    v0 = mul(c0, mk(mmag0 * cw0 + mpass0, mmag0 * sw0));
    v1 = mul(c1, mk(mmag1 * cw1 + mpass1, mmag1 * sw1));
    p0 = c0;
    p1 = c1;
}

// the same for one bin (the packed group's one-at-a-time ops)
__device__ __forceinline__ c2 pyramid_op_2band(c2 c, c2 p, const Spec &sp, float2 mt, float ms)
{
    const float mn2 = fminf(c.x * c.x + c.y * c.y, p.x * p.x + p.y * p.y);
    const float mb = fmaxf(mt.y, 0.0f);
    const float mmag = (mt.x * mt.x * mn2 < sp.tau2_nn ? 0.0f : mt.x) + (mb * mb * mn2 < sp.tau2_nn ? 0.0f : mb);
    const float mpass = ms - mmag;
    const c2 u = mul_conj(p, c);
    const float rev = fast_atan2(u.y, u.x) * sp.S_rev;
    const float cw = __builtin_amdgcn_cosf(rev), sw = __builtin_amdgcn_sinf(rev);
    return mul(c, mk(mmag * cw + mpass, mmag * sw));
}

template <int MODE>
__device__ __forceinline__ c2 standard_op_t(c2 c, c2 p, const Spec &sp, float2 mt)
{
    const float mn2 = fminf(c.x * c.x + c.y * c.y, p.x * p.x + p.y * p.y);
    if (mn2 < sp.tau2) return scale(c, sp.inv_nn);
    const float d = fast_atan2(p.y * c.x - p.x * c.y, p.x * c.x + p.y * c.y);
    const float ph = (d * mt.x) * sp.S;
    return scale(mul_c(c, mk(__cosf(ph), __sinf(ph))), sp.inv_nn);
}

template <int LOG2N> constexpr int k2_tab_entries() { return (1 << LOG2N) / 2 + 1; }
// Per-bin table slot of entry e (0 <= e <= N/2): entries e = w (mod C) are
// contiguous (slot (e mod C) Q + e / C, Q = ceil(entries / C)), so that a
// wave's bins fy = w + C (l + 64 j) (fft_bin: one residue w per wave) read
// consecutive slots, and the mirrored bins N - fy consecutive slots backwards:
// no bank conflicts (natural order: lanes 8 C bytes apart, 4-way at C = 4).
template <int LOG2N> constexpr int k2_tab_q() { return (k2_tab_entries<LOG2N>() + fft_c_v(LOG2N) - 1) / fft_c_v(LOG2N); }
template <int LOG2N> constexpr int k2_tab_slots() { return k2_tab_q<LOG2N>() * fft_c_v(LOG2N); }
template <int LOG2N>
__host__ __device__ constexpr int k2_tix(int e)
{
    constexpr int C = fft_c_v(LOG2N);
    return C == 1 ? e : (e % C) * k2_tab_q<LOG2N>() + e / C;
}

// MODE: MM_MODE_PYRAMID (dynamic masks), MM_MODE_STANDARD or MM_K2_PYR_TAB (tables)
template <int LOG2N, int MODE>
__device__ __forceinline__ c2 k2_op(c2 c, c2 p, int fx, int fy, const Spec &sp, const float2 *tab)
{
    constexpr int N = 1 << LOG2N;
    if constexpr (MODE == MM_MODE_PYRAMID) {
        return pyramid_op<LOG2N>(c, p, fx, fy, sp);
    } else {
        const float2 mt = tab[k2_tix<LOG2N>(fy <= N / 2 ? fy : N - fy)];
        if constexpr (MODE == MM_MODE_STANDARD) return standard_op_t<MODE>(c, p, sp, mt);
        else return pyramid_op_t<LOG2N>(c, p, fx, fy, sp, mt);
    }
}

// k_cols runs two columns per workgroup (whole 32-B Q pieces per tile row
// instead of one 8-B value per column).  At N = 4096 that is 16 waves with
// 123-148 KB of LDS, one workgroup per CU for the whole launch; one column per
// workgroup there (8 waves, two per CU) measured slower same-call (C3 k_cols
// 37.5 -> 38.6-39.0 us per frame: 16-B Q pieces).
template <int LOG2N> constexpr int k2_groups()
{
    return LOG2N >= 13 ? 1 : LOG2N >= 12 ? 2 : groups_at_least<LOG2N, MM_K2_GROUPS>();
}
// the steerable band-column kernel: one column per workgroup where one
// transform fills a workgroup (N >= 2048), else the transforms a 256-thread
// workgroup holds; its staged pieces are 32 B through the band rows' row
// groups of 4 (MM_SB_RROWS, mm_steer.hpp), and the workgroups of a CU run
// independently (two columns in one 1,024-thread workgroup synchronised 16
// waves per barrier: C3 O = 8 k_sb_cols 434 -> 380 us, 1080p 81.7 -> 69.4,
// profiles/r06h_sb_rows_layout_ab.txt).
template <int LOG2N> constexpr int sb_groups() { return groups_per_wg<LOG2N>(); }
// the steerable band-row kernel: row transforms per workgroup
template <int LOG2N> constexpr int sb_rows_groups() { return groups_per_wg<LOG2N>(); }
template <int LOG2N> constexpr int sb_rows_threads() { return sb_rows_groups<LOG2N>() * fft_T<LOG2N>(); }
template <int LOG2N> constexpr int sb_threads() { return sb_groups<LOG2N>() * fft_T<LOG2N>(); }
// K2's Q staging buffer (c2 slots written by rows, read back as float4
// pieces): slot i lives at i ^ (((i >> 4) & 1) << 1), i.e. float4 r at
// r ^ ((r >> 3) & 1).  The row writes of a 16-lane group (every other float4
// of a 16-float4 span) then cover all 32 banks once (linear: 2-way), and the
// ds_read_b128 groups still read 16 distinct 4-bank slots (tools/lds_banks.py).
__device__ __forceinline__ int k2_stg_swz(int i) { return i ^ (((i >> 4) & 1) << 1); }
__device__ __forceinline__ int k2_stg_swz4(int r) { return r ^ ((r >> 3) & 1); }
template <int LOG2N> constexpr int k2_threads() { return k2_groups<LOG2N>() * fft_T<LOG2N>(); }

// bytes of n columns' mask-sum arrays ([TS] floats each, rounded up to 16 B;
// pyramid tables with overlapping bands only)
template <int LOG2N, int MODE> constexpr size_t k2_msum_bytes(int n)
{
    return k2_msum<MODE>() ? ((sizeof(float) * (size_t)n * k2_tab_slots<LOG2N>()) + 15) / 16 * 16 : 0;
}
// k_cols' dynamic LDS, in layout order: the GPW exchange buffers, the GPW
// columns' tables and mask sums; then what only the packed group (block 0)
// uses: column N/2's table and mask sums and ldsX.  The staged Q pieces alias
// the exchange buffers.  Above 64 KiB at N = 2048 (77.8 KiB): two workgroups
// still fit a CU's 160 KiB.
template <int LOG2N, int MODE> constexpr size_t k2_lds_bytes()
{
    return (size_t)k2_groups<LOG2N>() *
               (sizeof(c2) * lds_complex<(1 << LOG2N)>() + sizeof(float2) * k2_tab_slots<LOG2N>()) +
           k2_msum_bytes<LOG2N, MODE>(k2_groups<LOG2N>()) +
           sizeof(float2) * k2_tab_slots<LOG2N>() + k2_msum_bytes<LOG2N, MODE>(1) + sizeof(c2) * 4;
}

// Columns f = 1..N/2-1 get one FFT group each.  The two real columns f = 0 and
// f = N/2 (row DFT bins that are real for real rows, so their column spectra are
// Hermitian in fy) share group 0 of block 0 as one complex column z = G0 + i*GN.
// The grid is then exactly N/2 groups (512 two-column workgroups at N=2048: one
// resident round at 2 WGs/CU, no one-group tail).  After the forward FFT the
// packed group unpacks F0, FN from Z(fy), Z(N-fy) (partner bins through LDS)
// and runs the same number of ops per thread as any other group: a thread's
// bins fy < N/2 (j < 4) carry column 0's op at fy, its bins fy > N/2 carry
// column N/2's op at N - fy; the two real bins of column N/2 (0 and N/2) are
// one extra op each for threads T/4 and 3T/4 (F_{t-1} and the result in ldsX).
// A second exchange recombines A = A0 + i AN per bin.
// (The packed block is the kernel's critical path: every block is resident at
// once, so its extra work is the kernel's.)
#ifndef MM_K2_OPX2G
#define MM_K2_OPX2G 8   // bins per scheduling group of the two-bin op (2, 4: K2 +3 %, +1 %)
#endif
#ifdef MM_K2_STAMPS
// Diagnostic build only: per-wave cycle totals of the frame-loop phases
// (s_memtime deltas), written by lane 0 with a vector store after the loop.
__device__ unsigned long long mm_k2_stamps[4096 * 8 * 8];
__device__ unsigned long long mm_k2_entry[4096 * 8];   // s_memrealtime at entry, per wave
__device__ unsigned long long mm_k2_exit[4096 * 8];    // ... after the last Q stores completed (vmcnt 0)
#define K2_STAMP(i)                                                      \
    do {                                                                 \
        const unsigned long long n_ = __builtin_amdgcn_s_memtime();      \
        st_acc[i] += n_ - st_prev;                                       \
        st_prev = n_;                                                    \
    } while (0)
#else
#define K2_STAMP(i) do { } while (0)
#endif
//
// The frame loop is instantiated twice (BLK0): block 0, whose group 0 is the
// packed group, runs the extra exchanges; every other block runs a loop with
// none of that code, so its register allocation is not shaped by the packed
// group's live values.
// The temporal state is G_{t-1}, K1's row spectra of the previous input frame
// (previousSourceTexture, .cs:142): every launch first runs `Gprev` through
// the forward transform as a passthrough frame (fr = -1), which sets F_{t-1}
// in registers bit for bit as the frame loop would have, then frames
// 0 .. nframes-1 of G, whose Q go to Q + fr * q_stride.
// A per-bin table entry from LDS as its own ds_read_b64 (lds_ld: not paired
// into a ds_read2_b64, which costs twice the LDS cycles on gfx950)
__device__ __forceinline__ float2 tab_ld(const float2 *p)
{
    const c2 v = lds_ld(reinterpret_cast<const c2 *>(p));
    return make_float2(v.x, v.y);
}

//
// HOLD (mm_set_hold, a held lane's stream form): the prime's F is the held
// reference F_ref and no later frame overwrites it, so every frame of the
// launch pairs with Gprev and the frames stop depending on each other.  The
// prime is the rolling form's (same runtime passthrough test: F_ref has the
// rolling prime's bits); what goes is every roll of the state: the generic
// op's prev[j] = v[j], the packed-pair ops' write-back (they get copies), the
// packed group's three branches and column N/2's real bins in ldsX.
template <int LOG2N, int MODE, bool BLK0, bool HOLD = false>
__device__ __forceinline__ void k_cols_body(const c2 *G, size_t g_stride, const c2 *Gprev, c2 *Q,
                                            size_t q_stride, int nframes, const Geo &g,
                                            const Spec &sp, const c2 *__restrict__ tw,
                                            const float2 *__restrict__ ktab, const float *__restrict__ kmsum,
                                            int blk, int nb_prio = 0)
{
    constexpr int N = 1 << LOG2N, T = fft_T<LOG2N>(), GPW = k2_groups<LOG2N>();
    constexpr int TS = k2_tab_slots<LOG2N>();
#ifdef MM_K2_STAMPS
    const unsigned long long st_entry = __builtin_amdgcn_s_memrealtime();
#endif
    extern __shared__ __attribute__((aligned(16))) c2 lds_all[];
    // group index: wave-uniform (scalar) when a group spans whole waves
    const int grp = T % 64 == 0 ? __builtin_amdgcn_readfirstlane(threadIdx.x / T) : threadIdx.x / T;
    const int t0 = threadIdx.x % T;
    c2 *lds = lds_all + grp * lds_complex<N>();
    // (N = 8192: the tables start past a DS instruction's 16-bit offset field;
    // as an opaque scalar the offset stays in one register, where the constant
    // cost a v_add per table read.  Not at N = 4096, whose tables start as far
    // in: there it cost the two-band instance 7 VALU.)
    int tab_off = GPW * lds_complex<N>();
    if constexpr (LOG2N == 13) asm volatile("" : "+s"(tab_off));
    float2 *tabs = reinterpret_cast<float2 *>(lds_all + tab_off);
    float2 *tab0 = tabs + grp * TS;
    // column N/2: F_{t-1} at its real bins 0 and N/2 and their results (two
    // threads of the packed group).  Its Q values are staged with column 0's:
    // the packed group's staging slot of a row holds (Q0, QN) (the inverse of
    // A0 + i AN; both real), split into the two columns' pieces at the store.
    // the bins' whole mask sums (tabled pyramid modes; two-band waves read them)
    float *ms0 = reinterpret_cast<float *>(tabs + GPW * TS) + grp * TS;
    // packed group only: column N/2's table, mask sums, ldsX
    float2 *tabN = reinterpret_cast<float2 *>(reinterpret_cast<uint8_t *>(tabs + GPW * TS) +
                                              k2_msum_bytes<LOG2N, MODE>(GPW));
    float *msN = reinterpret_cast<float *>(tabN + TS);
    c2 *ldsX = reinterpret_cast<c2 *>(reinterpret_cast<uint8_t *>(msN) + k2_msum_bytes<LOG2N, MODE>(1));
    const int f_raw = blk * GPW + grp;
    const bool valid = f_raw < N / 2;
    const int f = valid ? f_raw : N / 2 - 1;
    constexpr bool blk0 = BLK0;               // block 0 runs the extra exchanges
    const bool packed = blk0 && grp == 0;     // group owning columns 0 and N/2

    // G column of a frame.  Rows outside the image get an out-of-range buffer
    // offset: the range check returns 0 for them without a memory access (the
    // zero padding of PadTexture, .cs:358-381).  A frame's loads are issued
    // before the previous frame's Q stores, so the wait for them never waits
    // for those stores (one in-order vmcnt).  (Loading one frame ahead, 16
    // more VGPRs, measured no faster: the frame loop is bound by its barrier
    // and dependency-chain latencies, not by this load's.)
    c2 ga[8];
    float gb[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    // (buffer loads: 32-bit offsets, and kept in order with the buffer stores)
    // One buffer resource per column, its range the H image rows: row t + jT - y0
    // at byte offset (t - y0) 8 + j T 8, and rows outside the image (negative
    // offsets wrap to huge ones) fail the range check without any compare.
    auto load_g = [&](int fr, int t) {
        const int gfr = __builtin_amdgcn_readfirstlane(fr);   // uniform; -1: Gprev
        const c2 *Gc = gfr < 0 ? Gprev : G + (size_t)gfr * g_stride;
        const auto grs = __builtin_amdgcn_make_buffer_rsrc(const_cast<c2 *>(Gc) + (size_t)f * g.Hg, 0,
                                                           g.H * (int)sizeof(c2), 0x00020000);
        const unsigned o0 = (unsigned)(t - g.y0) * 8u;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
            const u32x2 a = __builtin_amdgcn_raw_buffer_load_b64(grs, o0 + (unsigned)(j * T * 8), 0, 0);
            ga[j] = mk(__uint_as_float(a.x), __uint_as_float(a.y));
        }
        if constexpr (blk0) {   // column N/2 (real) for the packed group's block only
            const auto nrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<c2 *>(Gc) + (size_t)(N / 2) * g.Hg, 0,
                                                               g.H * (int)sizeof(c2), 0x00020000);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                gb[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(nrs, o0 + (unsigned)(j * T * 8), 0, 0));
        }
    };
    // the prime's G_{t-1} loads first: their HBM latency overlaps the twiddle
    // loads and the table copy instead of following its barrier (one-frame
    // calls pay the prologue and the prime on every call)
    load_g(-1, t0);
    // twiddle bases of both FFTs, loaded once (issued under the table copy): no loads inside a frame but G's
    c2 wtw[kTwSlots];
#pragma unroll
    for (int i = 0; i < kTwSlots; ++i) wtw[i] = mk(1.0f, 0.0f);
    preload_twiddles_wl<LOG2N>(wtw, t0, tw);
    if constexpr (MODE != MM_MODE_PYRAMID) {
        // the column's table, evaluated once per parameter set by k_k2_table
        // (slot order): a copy instead of N/2+1 bin_static per group and launch
        const float2 *src0 = ktab + (size_t)f * TS;
        for (int e = t0; e < TS; e += T) tab0[e] = src0[e];
        if (packed) {
            const float2 *srcN = ktab + (size_t)(N / 2) * TS;
            for (int e = t0; e < TS; e += T) tabN[e] = srcN[e];
        }
        if constexpr (k2_msum<MODE>()) {
            const float *m0 = kmsum + (size_t)f * TS;
            for (int e = t0; e < TS; e += T) ms0[e] = m0[e];
            if (packed) {
                const float *mN = kmsum + (size_t)(N / 2) * TS;
                for (int e = t0; e < TS; e += T) msN[e] = mN[e];
            }
        }
        __syncthreads();
    }

    // waves whose bins all have at most one middle band (frame-invariant,
    // uniform) take the branch-free op
    // packed group: bin j's op column (0 or N/2) and bin within it
    auto pk_col0 = [&](int j, int fy) { return j < 4 || fy == N / 2; };
    bool wave_two_band = true;
    if constexpr (k2_tabled<MODE>()) {
        bool two = false;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int fy = fft_bin<LOG2N>(t0, j);
            if (packed && !pk_col0(j, fy)) two |= !__builtin_signbit(tabN[k2_tix<LOG2N>(N - fy)].y);
            else two |= !__builtin_signbit(tab0[k2_tix<LOG2N>(fy <= N / 2 ? fy : N - fy)].y);
        }
        if (packed && t0 == 0)
            two |= !__builtin_signbit(tabN[k2_tix<LOG2N>(0)].y) || !__builtin_signbit(tabN[k2_tix<LOG2N>(N / 2)].y);
        wave_two_band = __any(two);
    }
    // F_{t-1}: set by the passthrough frame fr = -1 (Gprev)
    c2 prev[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) prev[j] = mk(0.0f, 0.0f);

    // per-bin table bases of a regular group's bins (regular_op): bin j is
    // fy = fy0 + j N/8 (fy0 = fft_bin(t, 0)), table entry fy for j < 4, N - fy
    // for j >= 4; N/8 is a multiple of C, so both are slots of two
    // frame-invariant bases plus immediates (k2_tix): entry fy0 + m C at slot
    // k2_tix(fy0) + m, entry M - fy0 (M a multiple of C) at slot
    // k2_tix(C - w) - 1 - fy0 / C + M / C for w = fy0 mod C > 0.
    // (hoisted out of the frame loop where registers allow: N >= 2048, TK == 2;
    // smaller N recompute them per frame from the opaque lane index)
    constexpr bool HOIST = q_tile<LOG2N>() == 2;
    const int hfy0 = fft_bin<LOG2N>(t0, 0);
    const int hw = hfy0 % fft_c_v(LOG2N);
    const float2 *tlo0 = tab0 + k2_tix<LOG2N>(hfy0);
    const float2 *thi0 = tab0 + (hw ? k2_tix<LOG2N>(fft_c_v(LOG2N) - hw) - 1 : 0) - hfy0 / fft_c_v(LOG2N);

    constexpr int TK = q_tile<LOG2N>(), BLK = GPW * TK / 2;   // float4 per tile row
    constexpr int NST = (N * GPW / 2 + GPW * T - 1) / (GPW * T);   // store slots per thread (Hq <= N)
    const int fb = blk * GPW, nq = (g.Hq / TK) * BLK;
    c2 *stg = lds_all;   // staged Q pieces of a frame: [row pair][GPW][TK], over the exchange buffers
    bool staged = false;   // stg holds the previous frame's pieces (uniform)
    // Canvas-row staging (TK == 2, rb even, no list row wrapping: every
    // geometry but H close to N): the inverse transform's rows n = t + jT go
    // to LDS unconditionally at slot(n) = ((n/2) GPW + grp) TK + n%2 (one base
    // + immediates, no per-row checks), and the Q stores read list row pair kt
    // at canvas pair kt + rb/2.  Otherwise list-row staging (rows of [0, Hq)).
    const bool cstage = TK == 2 && (g.rb & 1) == 0 && g.rb >= 0 && g.rb + g.Hq <= N;
    const int rd_off = cstage ? (g.rb / 2) * GPW : 0;   // float4 pieces
    // frame-invariant per-thread Q store offsets (loop invariant: computed
    // from t0, not the opaque t below); a frame with nothing staged stores
    // through an empty buffer range instead
    unsigned so_st[NST];
#pragma unroll
    for (int i = 0; i < NST; ++i) {
        const int e = grp * T + t0 + i * GPW * T;
        const int kt = e / BLK, r = e - kt * BLK;
        const bool ok = e < nq && (GPW <= N / 2 || fb + (2 * r) / TK < N / 2);   // tiny N: fewer columns than groups
        so_st[i] = ok ? (unsigned)((kt * g.Qs + fb) * TK + 2 * r) * 8u : 0x80000000u;
    }
    // (k2_stg_swz: float4 r at r ^ ((r >> 3) & 1); + i GPW T keeps bit 3)
    const float4 *rd_base = reinterpret_cast<const float4 *>(stg) + k2_stg_swz4(grp * T + t0 + rd_off);

    // One straight path per iteration: G loads of frame fr, then the Q stores
    // of frame fr-1 from the staging buffer (exactly NST buffer stores per
    // thread; slots past the end are dropped by the range check), then frame
    // fr, whose first use of the loads waits with vmcnt(NST) and never for the
    // stores.
#ifdef MM_K2_STAMPS
    unsigned long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long st_prev = __builtin_amdgcn_s_memtime();
    st_acc[7] = __builtin_amdgcn_s_memrealtime();   // loop start (100 MHz, device-wide)
#endif
    // One frame of the loop.  The prime (fr = -1) runs as its own instance
    // ahead of the loop, so the frame loop itself is compiled with no
    // passthrough branch: in one shared body the branch merge made the
    // compiler copy the FFT outputs twice per frame (once for the merge, once
    // into the loop-carried F_{t-1}: 32 v_mov; K2 -2 % at 1080p, -3 % at
    // 2160p same-call).  The prime keeps a RUNTIME passthrough test (fr is
    // made opaque): an instance specialised on a constant fr = -1 computed an
    // F_{t-1} 1 ulp away from the in-loop one, which broke the bitwise
    // equality of one-frame calls, tails, ring hand-offs and batches.
    // OPK: the regular groups' op, fixed per loop instance (the one-band op or
    // the rest, chosen once per wave: wave_two_band is frame-invariant), so the
    // register allocation of the one-band loop is not shaped by the generic
    // op's live values; -1: chosen per frame at run time (block 0)
    auto frame_iter = [&](const int fr, auto opk_c) __attribute__((always_inline)) -> bool {
        constexpr int OPK = decltype(opk_c)::value;
        // Opaque per-iteration copy of the lane index: stops LICM from hoisting
        // every t-derived LDS address and twiddle of both FFTs out of the frame
        // loop (that pinned ~200 VGPRs and capped occupancy at 1 wave/SIMD).
        int t = t0;
        asm volatile("" : "+v"(t));
        // Two workgroups share a CU for the whole launch and the SIMD arbiter
        // favours the older one (issue priority, then age): it ran ahead and
        // left the younger one alone for the last third (phase stamps: loop
        // times 917 vs 1357 us per 100 frames).  Alternating the priority
        // every frame between the first-dispatched half of the grid and the
        // second keeps a pair in step (1082..1305 us).
        // Block 0 (the packed group's extra exchanges: the kernel's critical
        // path, phase stamps) keeps the highest priority throughout (same-call
        // A/B: ≈ 1 % over alternating it too, and over raising the packed group only).
        if (blk0) __builtin_amdgcn_s_setprio(3);
        else if ((fr ^ ((int)blockIdx.x >= nb_prio / 2 ? 1 : 0)) & 1) __builtin_amdgcn_s_setprio(2);
        else __builtin_amdgcn_s_setprio(1);
        // (Gprev's loads: issued before the prologue; later frames' mid-iteration)
        K2_STAMP(0);
        __builtin_amdgcn_sched_barrier(0);   // keep the stores behind the loads
        {
            float4 sv[NST];
#pragma unroll
            for (int i = 0; i < NST; ++i) sv[i] = rd_base[i * GPW * T];   // (slots past the staging: unused)
            // staging read before this frame's FFT rewrites the buffers
            __syncthreads();
            const int qfr = __builtin_amdgcn_readfirstlane(fr > 0 ? fr - 1 : 0);   // uniform
            const auto qrs = __builtin_amdgcn_make_buffer_rsrc(
                Q + (size_t)qfr * q_stride, 0, staged ? (int)(q_stride * sizeof(c2)) : 0, 0x00020000);
            unsigned so[NST];
#pragma unroll
            for (int i = 0; i < NST; ++i) {
                if constexpr (HOIST) {
                    so[i] = so_st[i];
                } else {   // per frame from the opaque t (registers)
                    const int e = grp * T + t + i * GPW * T;
                    const int kt = e / BLK, r = e - kt * BLK;
                    const bool ok = e < nq && (GPW <= N / 2 || fb + (2 * r) / TK < N / 2);
                    so[i] = ok ? (unsigned)((kt * g.Qs + fb) * TK + 2 * r) * 8u : 0x80000000u;
                }
            }
#pragma unroll
            for (int i = 0; i < NST; ++i) {
                typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
                u32x4 d = {__float_as_uint(sv[i].x), __float_as_uint(sv[i].y), __float_as_uint(sv[i].z),
                           __float_as_uint(sv[i].w)};
                if constexpr (blk0) {
                    // a piece of the packed group (column 0: group 0 of block 0)
                    // holds (Q0, QN) per row: column 0 gets the real parts, column
                    // N/2 (same rows, N/2 bins further in the tile row) the rest
                    const int e = grp * T + t + i * GPW * T;
                    if ((2 * (e % BLK)) / TK == 0) {
                        const u32x4 dn = {d.y, 0u, d.w, 0u};
                        d.y = 0u;
                        d.w = 0u;
                        __builtin_amdgcn_raw_buffer_store_b128(dn, qrs, so[i] + (unsigned)((N / 2) * TK * 8), 0, 0);
                    }
                }
                __builtin_amdgcn_raw_buffer_store_b128(d, qrs, so[i], 0, 0);
            }
        }
        K2_STAMP(1);
        if (fr == nframes) return false;
        c2 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j)   // G[0][r], G[N/2][r] are real (exact zero imaginary parts)
            v[j] = packed ? mk(ga[j].x, gb[j]) : ga[j];
        const bool pass_frame = fr < 0;   // the prime (fr = -1)
        // the prime's successor (frame 0) loads now, under the prime's transform
        // (the prime has no op, so its "after the op" slot below came one
        // transform later; a one-frame call waits on these loads next)
        if (pass_frame) load_g(nframes > 0 ? 0 : -1, t);
        // opaque per-iteration copy of the twiddle bases (same reason as t: the
        // products of their powers must not be hoisted into live registers)
        c2 wt[kTwSlots];
#pragma unroll
        for (int i = 0; i < kTwSlots; ++i) {
            wt[i] = wtw[i];
            if (tw_slot_used_wl(LOG2N, i)) asm volatile("" : "+v"(wt[i]));
        }
        // hold: F_ref is loop-invariant, and so is what the ops derive from it
        // alone (|F_ref|^2 per bin): the compiler hoists that, which saves the
        // VALU per frame and keeps up to 12 more VGPRs live than the rolling
        // twin has.  That fits the 128 of four waves per SIMD without a spill
        // at every size but N = 8192 (tabled op: 6 spilled), where an opaque
        // per-iteration copy in place (no v_mov) undoes the hoisting.  (At the
        // other sizes the copy costs registers instead: the pairs it pins at
        // N = 2048 made three of the four instances spill.)
        if constexpr (HOLD && LOG2N == 13) {
#pragma unroll
            for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(prev[j]));
        }
        K2_STAMP(2);
        MM_MARK("M1_fwd_start");
        fft_dif<LOG2N, -1>(v, t, lds, wt);
        MM_MARK("M2_fwd_end");
        K2_STAMP(3);
        // the spectral op of a regular group (all groups but the packed one)
        auto regular_op = [&]() {
            if (pass_frame) {
#pragma unroll
                for (int j = 0; j < 8; ++j) prev[j] = v[j];
            } else if (k2_one_band_op<MODE>() && (OPK == 1 || (OPK < 0 && !wave_two_band))) {
                // no bin of this wave has two middle bands: branch-free op, two
                // bins per packed op
                // bin j: fy = fy0 + j N/8 (fy0 = fft_bin(t, 0)), table entry fy
                // for j < 4, N - fy for j >= 4 (fy <= N/2 exactly for j < 4).
                // N/8 is a multiple of C, so both are slots of two per-frame
                // bases plus immediates (k2_tix): entry fy0 + m C at slot
                // k2_tix(fy0) + m, entry M - fy0 (M a multiple of C) at slot
                // k2_tix(C - w) - 1 - fy0 / C + M / C for w = fy0 mod C > 0.
                constexpr int C = fft_c_v(LOG2N);
                const int fy0 = fft_bin<LOG2N>(HOIST ? t0 : t, 0);   // frame-invariant (hoisted: t0)
                const int w = fy0 % C;
                const float2 *tlo = HOIST ? tlo0 : tab0 + k2_tix<LOG2N>(fy0);
                const float2 *thi = HOIST ? thi0 : tab0 + (w ? k2_tix<LOG2N>(C - w) - 1 : 0) - fy0 / C;
#pragma unroll
                for (int j = 0; j < 8; j += 2) {   // two bins per packed op
                    if (j % MM_K2_OPX2G == 0) __builtin_amdgcn_sched_barrier(0);
                    const float2 mt0 = tab_ld(j < 4 ? tlo + j * (N / 8) / C : thi + (N - j * (N / 8)) / C);
                    const float2 mt1 = tab_ld(j + 1 < 4 ? tlo + (j + 1) * (N / 8) / C : thi + (N - (j + 1) * (N / 8)) / C);
                    if constexpr (HOLD) {   // F_ref stays: the op rolls copies
                        c2 p0 = prev[j], p1 = prev[j + 1];
                        pyramid_op_1band_x2(v[j], p0, mt0, v[j + 1], p1, mt1, sp);
                    } else {
                        pyramid_op_1band_x2(v[j], prev[j], mt0, v[j + 1], prev[j + 1], mt1, sp);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            } else if (MODE == MM_K2_PYR_TAB2) {
                // a bin of this wave has two middle bands (L = 6 layouts): the
                // branch-free two-band op, same table addressing + mask sums
                constexpr int C = fft_c_v(LOG2N);
                const int fy0 = fft_bin<LOG2N>(HOIST ? t0 : t, 0);
                const int w = fy0 % C;
                const float2 *tlo = HOIST ? tlo0 : tab0 + k2_tix<LOG2N>(fy0);
                const float2 *thi = HOIST ? thi0 : tab0 + (w ? k2_tix<LOG2N>(C - w) - 1 : 0) - fy0 / C;
                const float *mlo = ms0 + (tlo - tab0), *mhi = ms0 + (thi - tab0);
#pragma unroll
                for (int j = 0; j < 8; j += 2) {
                    if (j % MM_K2_OPX2G == 0) __builtin_amdgcn_sched_barrier(0);
                    const int i0 = j < 4 ? j * (N / 8) / C : (N - j * (N / 8)) / C;
                    const int i1 = j + 1 < 4 ? (j + 1) * (N / 8) / C : (N - (j + 1) * (N / 8)) / C;
                    const float2 mt0 = tab_ld(j < 4 ? tlo + i0 : thi + i0), mt1 = tab_ld(j + 1 < 4 ? tlo + i1 : thi + i1);
                    const float s0 = j < 4 ? mlo[i0] : mhi[i0], s1 = j + 1 < 4 ? mlo[i1] : mhi[i1];
                    if constexpr (HOLD) {
                        c2 p0 = prev[j], p1 = prev[j + 1];
                        pyramid_op_2band_x2(v[j], p0, mt0, s0, v[j + 1], p1, mt1, s1, sp);
                    } else {
                        pyramid_op_2band_x2(v[j], prev[j], mt0, s0, v[j + 1], prev[j + 1], mt1, s1, sp);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    // one bin at a time: keeps the 8 op instances from being interleaved
                    __builtin_amdgcn_sched_barrier(0);
                    const c2 a = k2_op<LOG2N, MODE>(v[j], prev[j], f, fft_bin<LOG2N>(t, j), sp, tab0);
                    if constexpr (!HOLD) prev[j] = v[j];
                    v[j] = a;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        if constexpr (blk0) {
            // packed group (see above the kernel).  First every wave leaves its
            // fft_dif region; then Z of every bin to LDS for the partner reads.
            __syncthreads();
            if (packed) {
#pragma unroll
                for (int j = 0; j < 8; ++j) lds[zslot<LOG2N>(fft_bin<LOG2N>(t, j))] = v[j];
            }
            __syncthreads();
            // v[j] becomes A0(fy) (j < 4) / AN(N - fy) (j >= 4)
            if (packed) {
                // unpack every bin (partner Z(N - fy) from LDS), then the ops
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int fy = fft_bin<LOG2N>(t, j);
                    const c2 z = v[j], m = lds[zslot<LOG2N>((N - fy) & (N - 1))];
                    const c2 f0 = mk(0.5f * (z.x + m.x), 0.5f * (z.y - m.y));    // F0(fy)
                    const c2 fn = mk(0.5f * (z.y + m.y), -0.5f * (z.x - m.x));   // FN(fy)
                    v[j] = pk_col0(j, fy) ? f0 : mk(fn.x, -fn.y);                // or FN(N - fy)
                }
                if (!pass_frame) {
                    if (k2_one_band_op<MODE>() && !wave_two_band) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            __builtin_amdgcn_sched_barrier(0);   // one bin at a time: registers
                            const int fy = fft_bin<LOG2N>(t, j);
                            const c2 c = v[j];
                            const float2 mt = pk_col0(j, fy) ? tab0[k2_tix<LOG2N>(fy)] : tabN[k2_tix<LOG2N>(N - fy)];
                            v[j] = pyramid_op_1band(c, prev[j], sp, mt);
                            if constexpr (!HOLD) prev[j] = c;
                        }
                    } else if (MODE == MM_K2_PYR_TAB2) {   // two-band waves
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            __builtin_amdgcn_sched_barrier(0);
                            const int fy = fft_bin<LOG2N>(t, j);
                            const bool c0 = pk_col0(j, fy);
                            const int ix = k2_tix<LOG2N>(c0 ? fy : N - fy);
                            const c2 c = v[j];
                            v[j] = pyramid_op_2band(c, prev[j], sp, c0 ? tab0[ix] : tabN[ix], c0 ? ms0[ix] : msN[ix]);
                            if constexpr (!HOLD) prev[j] = c;
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            __builtin_amdgcn_sched_barrier(0);
                            const int fy = fft_bin<LOG2N>(t, j);
                            const c2 c = v[j];
                            v[j] = pk_col0(j, fy) ? k2_op<LOG2N, MODE>(c, prev[j], 0, fy, sp, tab0)
                                                  : k2_op<LOG2N, MODE>(c, prev[j], N / 2, N - fy, sp, tabN);
                            if constexpr (!HOLD) prev[j] = c;
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) prev[j] = v[j];
                }
                // column N/2's real bins 0 and N/2: FN = Im Z there (Z(0) and
                // Z(N/2) are their own partners, still in LDS), op against
                // F_{t-1} in ldsX[0..1]; AN to ldsX[2..3] for thread 0's
                // recombine.  Threads T/4 and 3T/4 (waves 1 and 3 at N = 2048,
                // not wave 0, which holds fy = 0 and N/2 in the recombine).
#pragma unroll
                for (int x = 0; x < 2; ++x) {
                    if (t == (x ? 3 * T / 4 : T / 4)) {
                        const int fyx = x ? N / 2 : 0;
                        const c2 z = lds[zslot<LOG2N>(fyx)];
                        const c2 fn = mk(0.5f * (z.y + z.y), -0.5f * (z.x - z.x));
                        if (!pass_frame) ldsX[2 + x] = k2_op<LOG2N, MODE>(fn, ldsX[x], N / 2, fyx, sp, tabN);
                        if (!HOLD || pass_frame) ldsX[x] = fn;
                    }
                }
            } else {
                regular_op();   // the block's other group, between the same barriers
            }
            __syncthreads();   // partner reads of Z done: the buffer takes the ops
            // A0 at zslot_h(fy), AN at ZH + zslot_h(fy) (fy <= N/2): each
            // wave's writes and reads are consecutive slots (tools/lds_banks.py)
            constexpr int ZH = zslot_h_size<LOG2N>();
            static_assert(2 * ZH <= lds_complex<N>(), "recombine exchange fits the buffer");
            if (packed && !pass_frame) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int fy = fft_bin<LOG2N>(t, j);
                    if (pk_col0(j, fy)) lds[zslot_h<LOG2N>(fy)] = v[j];
                    else lds[ZH + zslot_h<LOG2N>(N - fy)] = v[j];
                }
            }
            __syncthreads();
            if (packed && !pass_frame) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int fy = fft_bin<LOG2N>(t, j);
                    c2 a0, an;
                    if (pk_col0(j, fy)) {   // A(fy) = A0(fy) + i AN(fy)
                        a0 = v[j];
                        an = fy == 0 ? ldsX[2] : (fy == N / 2 ? ldsX[3] : lds[ZH + zslot_h<LOG2N>(fy)]);
                    } else {                // A(fy) = conj A0(N-fy) + i conj AN(N-fy)
                        const c2 b = lds[zslot_h<LOG2N>(N - fy)];
                        a0 = mk(b.x, -b.y);
                        an = mk(v[j].x, -v[j].y);
                    }
                    v[j] = mk(a0.x - an.y, a0.y + an.x);
                }
            }
            __syncthreads();   // the inverse FFT rewrites the buffer
        }
        if constexpr (!blk0) regular_op();
        // next frame's G loads now: they land during this frame's inverse
        // transform, staging and Q stores instead of stalling the next frame
        // at its top (same-call K2 8.94 -> 8.33 us/frame, profiles/r03_abv.txt;
        // the op's registers are free again here: no spill at 123 VGPRs)
        if (!pass_frame) load_g(fr + 1 < nframes ? fr + 1 : nframes - 1, t);
        staged = !pass_frame;
        if (!pass_frame) {
        K2_STAMP(4);
        MM_MARK("M3_inv_start");
        fft_dit<LOG2N, +1>(v, t, lds, wt);   // natural row order again
        MM_MARK("M4_inv_end");
        K2_STAMP(5);
        __syncthreads();   // every wave past its exchange reads: the staging overwrites them
        // Q is stored by row pairs (q_index) so that K3 reads each of its two
        // rows' values as one 16-B piece per bin, contiguous across the wave (a
        // column-major Q made K3's 16-B gathers cost it 4 of its 7 us/frame at
        // 1080p).  The GPW columns of the workgroup are transposed through LDS
        // (over the exchange buffers) and leave as one contiguous GPW*16-byte piece
        // per row pair; same-XCD workgroups complete the 128-B lines.
        // Rows that never wrap (rb >= 0, rb + Hq <= N, every geometry but H
        // close to N): list row k = t + jT - rb, staging slot s(k) = s(k0) + jT GPW
        // (T a multiple of TK): one base and immediate offsets.
        if (cstage) {
            const int s0 = ((t >> 1) * GPW + grp) * TK + (t & 1);   // T even: (t + jT)/2 = t/2 + jT/2
            if (valid) {
#pragma unroll
                for (int j = 0; j < 8; ++j) stg[k2_stg_swz(s0) + j * (T / 2) * GPW * TK] = v[j];   // packed: (Q0, QN)
            }
        } else if (T % TK == 0 && g.rb >= 0 && g.rb + g.Hq <= N) {
            const int k0 = t - g.rb;   // may be negative: floor division below
            const int s0 = ((k0 >> ilog2c(TK)) * GPW) * TK + (k0 & (TK - 1));
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (valid && (unsigned)(k0 + j * T) < (unsigned)g.Hq)
                    stg[k2_stg_swz(s0 + j * T * GPW + TK * grp)] = v[j];   // packed (grp 0): (Q0, QN)
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = (t + j * T - g.rb + 2 * N) & (N - 1);
                if (valid && k < g.Hq) stg[k2_stg_swz(((k / TK) * GPW) * TK + (k % TK) + TK * grp)] = v[j];
            }
        }
        }   // !pass_frame
        __syncthreads();   // staged pieces complete (stored at the top of the next iteration)
        K2_STAMP(6);
        return true;
    };
    auto run_frames = [&](auto opk_c) __attribute__((always_inline)) {
        {
            int fr_prime = -1;   // opaque: the prime instance keeps the runtime passthrough test
            asm volatile("" : "+s"(fr_prime));
            frame_iter(fr_prime, opk_c);
        }
        for (int fr = 0;; ++fr)
            if (!frame_iter(fr, opk_c)) break;   // (fr >= 0 here: no passthrough branch)
    };
    if constexpr (blk0 || !k2_one_band_op<MODE>()) run_frames(std::integral_constant<int, -1>());
    else if (!wave_two_band) run_frames(std::integral_constant<int, 1>());
    else run_frames(std::integral_constant<int, 0>());
#ifdef MM_K2_STAMPS
    st_acc[7] = (__builtin_amdgcn_s_memrealtime() - st_acc[7]) << 32 | (st_acc[7] & 0xffffffffull);
    __builtin_amdgcn_s_waitcnt(0);   // every load and store of the wave completed
    const unsigned long long st_exit = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x % 64 == 0) {
        // k_cols_tail's workgroups (one per frame) after k_cols's 4096 waves
        const int w = (blk0 && nframes == 1 && gridDim.x < 512 ? 4096 : 0) +
                      blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
        for (int i = 0; i < 8; ++i) mm_k2_stamps[w * 8 + i] = st_acc[i];
        mm_k2_entry[w] = st_entry;
        mm_k2_exit[w] = st_exit;
    }
#endif
}

#ifndef MM_K2_WAVES
#define MM_K2_WAVES 4
#endif

template <int LOG2N, int MODE>
__global__ __launch_bounds__(k2_threads<LOG2N>()) __attribute__((amdgpu_waves_per_eu(MM_K2_WAVES)))
void k_cols(const c2 *G, size_t g_stride, const c2 *Gprev, c2 *Q, size_t q_stride,   // not restrict: G loads must stay ahead of Q stores
            int nframes, Geo g, Spec sp, const c2 *__restrict__ tw, const float2 *__restrict__ ktab,
            const float *__restrict__ kmsum, int nframes_blk0, int tail_blocks, int ktail)
{
    // Blocks nb .. nb + tail_blocks - 1 (tail_blocks <= nb / 2) are tails: the
    // last ktail frames of the columns of second-half block nb/2 + i, which
    // stops that many frames early.  A CU's second workgroup (the younger,
    // second half of the dispatch) runs behind its first all launch long
    // (phase stamps: first half done at ~825 us, second at ~1,045 us per 100
    // frames); its tail starts in the slot the first one frees, primed with the
    // frame before its first (the state is a pure function of that frame).
    const int nb = gridDim.x - tail_blocks;
    const bool tail = (int)blockIdx.x >= nb;
    const int p = tail ? nb / 2 + ((int)blockIdx.x - nb) : (int)blockIdx.x;
    // same-XCD blocks own consecutive columns, so the pieces of one 128-B Q line
    // are merged in one L2 (split over XCDs they left as partial-line writes)
    const int blk = xcd_remap(p, nb);
    if (blk == 0) {   // the packed block stops nframes_blk0 frames in (k_cols_tail)
        k_cols_body<LOG2N, MODE, true>(G, g_stride, Gprev, Q, q_stride, nframes_blk0, g, sp, tw, ktab, kmsum, blk, nb);
    } else {
        const int f0 = tail ? nframes - ktail : 0;
        const int nf = tail ? ktail : (p >= nb / 2 && p - nb / 2 < tail_blocks ? nframes - ktail : nframes);
        k_cols_body<LOG2N, MODE, false>(G + (size_t)f0 * g_stride, g_stride,
                                        tail ? G + (size_t)(f0 - 1) * g_stride : Gprev,
                                        Q + (size_t)f0 * q_stride, q_stride, nf, g, sp, tw, ktab, kmsum, blk, nb);
    }
}

// k_cols against a held reference (mm_set_hold): every frame of the launch
// pairs with Gprev, which each workgroup transforms once, in its prime, and no
// frame overwrites (k_cols_body's HOLD form).  The grid and the tail split are
// k_cols's; a tail block primes with Gprev like every other workgroup, not
// with the frame before its first.  (A kernel of its own, not a template
// parameter of k_cols: the rolling instances keep their symbols and text.)
template <int LOG2N, int MODE>
__global__ __launch_bounds__(k2_threads<LOG2N>()) __attribute__((amdgpu_waves_per_eu(MM_K2_WAVES)))
void k_cols_hold(const c2 *G, size_t g_stride, const c2 *Gprev, c2 *Q, size_t q_stride,   // not restrict, as k_cols
                 int nframes, Geo g, Spec sp, const c2 *__restrict__ tw, const float2 *__restrict__ ktab,
                 const float *__restrict__ kmsum, int nframes_blk0, int tail_blocks, int ktail)
{
    const int nb = gridDim.x - tail_blocks;
    const bool tail = (int)blockIdx.x >= nb;
    const int p = tail ? nb / 2 + ((int)blockIdx.x - nb) : (int)blockIdx.x;
    const int blk = xcd_remap(p, nb);
    if (blk == 0) {
        k_cols_body<LOG2N, MODE, true, true>(G, g_stride, Gprev, Q, q_stride, nframes_blk0, g, sp, tw, ktab, kmsum, blk, nb);
    } else {
        const int f0 = tail ? nframes - ktail : 0;
        const int nf = tail ? ktail : (p >= nb / 2 && p - nb / 2 < tail_blocks ? nframes - ktail : nframes);
        k_cols_body<LOG2N, MODE, false, true>(G + (size_t)f0 * g_stride, g_stride, Gprev,
                                              Q + (size_t)f0 * q_stride, q_stride, nf, g, sp, tw, ktab, kmsum, blk, nb);
    }
}

// The packed block's last frames, one workgroup per frame, after k_cols.
// Block 0 carries the packed group's extra exchanges and is k_cols's critical
// path, so the other blocks would idle at the end of the launch (rocprofv3:
// k_cols 1,016 us per 100 frames alone; 939 us + 24.5 us of k_cols_tail with
// the last 30 frames moved, 940 + 24.6 with 45: the 30 % default is past the
// point where block 0 stops being the critical path).  The state is a pure
// function of the previous input frame (.cs:142), so workgroup i primes with
// frame f0 + i - 1 (its passthrough frame sets F_{t-1} exactly as the frame
// loop would: bitwise the same outputs) and then runs frame f0 + i.
template <int LOG2N, int MODE>
__global__ __launch_bounds__(k2_threads<LOG2N>()) __attribute__((amdgpu_waves_per_eu(MM_K2_WAVES)))
void k_cols_tail(const c2 *G, size_t g_stride, const c2 *Gprev, c2 *Q, size_t q_stride, int f0, Geo g, Spec sp,
                 const c2 *__restrict__ tw, const float2 *__restrict__ ktab, const float *__restrict__ kmsum)
{
    const int fr = f0 + (int)blockIdx.x;   // frame 0 primes with the state slot
    k_cols_body<LOG2N, MODE, true>(G + (size_t)fr * g_stride, g_stride,
                                   fr > 0 ? G + (size_t)(fr - 1) * g_stride : Gprev,
                                   Q + (size_t)fr * q_stride, q_stride, 1, g, sp, tw, ktab, kmsum, 0);
}

// k_cols_tail against a held reference: every workgroup primes with Gprev.
// One frame per workgroup rolls nothing, so the body is the rolling one: a
// one-frame call's, on the held state.
template <int LOG2N, int MODE>
__global__ __launch_bounds__(k2_threads<LOG2N>()) __attribute__((amdgpu_waves_per_eu(MM_K2_WAVES)))
void k_cols_tail_hold(const c2 *G, size_t g_stride, const c2 *Gprev, c2 *Q, size_t q_stride, int f0, Geo g, Spec sp,
                      const c2 *__restrict__ tw, const float2 *__restrict__ ktab, const float *__restrict__ kmsum)
{
    const int fr = f0 + (int)blockIdx.x;
    k_cols_body<LOG2N, MODE, true>(G + (size_t)fr * g_stride, g_stride, Gprev,
                                   Q + (size_t)fr * q_stride, q_stride, 1, g, sp, tw, ktab, kmsum, 0);
}

// One frame of each of gridDim.y independent streams (mm_process_lanes): lane
// y's G_t, G_{t-1} and Q lie y slots into G, Gprev and Q.  Workgroup (x, y) is
// the one-frame call's k_cols workgroup x on lane y's pointers: the same body
// instances, nframes = 1, so a lane's Q is bitwise a one-frame call's.  Block x
// lands on XCD x % 8 within a lane only where gridDim.x % 8 == 0 (a 2-D grid
// dispatches x fastest); elsewhere a lane's same-XCD blocks no longer own
// consecutive columns, which costs the merging of Q lines, not results.
template <int LOG2N, int MODE>
__global__ __launch_bounds__(k2_threads<LOG2N>()) __attribute__((amdgpu_waves_per_eu(MM_K2_WAVES)))
void k_cols_lanes(const c2 *G, size_t g_stride, const c2 *Gprev, c2 *Q, size_t q_stride,   // not restrict, as k_cols
                  Geo g, Spec sp, const c2 *__restrict__ tw, const float2 *__restrict__ ktab,
                  const float *__restrict__ kmsum)
{
    const int nb = gridDim.x;
    const int blk = xcd_remap((int)blockIdx.x, nb);
    const size_t go = (size_t)blockIdx.y * g_stride;
    c2 *Ql = Q + (size_t)blockIdx.y * q_stride;
    if (blk == 0) k_cols_body<LOG2N, MODE, true>(G + go, g_stride, Gprev + go, Ql, q_stride, 1, g, sp, tw, ktab, kmsum, blk, nb);
    else k_cols_body<LOG2N, MODE, false>(G + go, g_stride, Gprev + go, Ql, q_stride, 1, g, sp, tw, ktab, kmsum, blk, nb);
}

// Index of the r-th set bit of m (r < popcount(m)): a binary search over the
// halves' bit counts.  m and r are workgroup-uniform where k_cols_lanes_sel
// calls it (a kernel argument and blockIdx.y), so the six steps are scalar work.
__device__ __forceinline__ int nth_set_bit(unsigned long long m, int r)
{
    int at = 0;
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
        const int c = __popcll(m & ((1ull << w) - 1));
        if (r >= c) {
            r -= c;
            m >>= w;
            at += w;
        }
    }
    return at;
}

// k_cols_lanes over a subset of the lanes, each with a bank of its own
// (mm_process_lanes_mask with a mask that leaves lanes out, or lanes whose
// bank bits differ): workgroup (x, y) takes the lane of the y-th set bit of
// `sel`.  LG holds two banks of `lanes` G slots; bit k of `banks` is the bank
// of lane k's G_{t-1}, its G_t is in the other bank's slot k, its Q at
// Q + k * q_stride.  From there it is k_cols_lanes: the same body instances,
// nframes = 1.  The selection costs a scalar prologue before the first load
// (0.05-0.1 us per lane-frame at 1080p), which is why calls of all lanes with
// one bank bit keep k_cols_lanes.
template <int LOG2N, int MODE>
__global__ __launch_bounds__(k2_threads<LOG2N>()) __attribute__((amdgpu_waves_per_eu(MM_K2_WAVES)))
void k_cols_lanes_sel(const c2 *LG, size_t g_stride, c2 *Q, size_t q_stride,   // not restrict, as k_cols
                      unsigned long long sel, unsigned long long banks, int lanes,
                      Geo g, Spec sp, const c2 *__restrict__ tw, const float2 *__restrict__ ktab,
                      const float *__restrict__ kmsum)
{
    const int nb = gridDim.x;
    const int blk = xcd_remap((int)blockIdx.x, nb);
    const int lane = nth_set_bit(sel, (int)blockIdx.y);
    const int pb = (int)((banks >> lane) & 1);
    const c2 *G = LG + (size_t)(lanes * (1 - pb) + lane) * g_stride;
    const c2 *Gprev = LG + (size_t)(lanes * pb + lane) * g_stride;
    c2 *Ql = Q + (size_t)lane * q_stride;
    if (blk == 0) k_cols_body<LOG2N, MODE, true>(G, g_stride, Gprev, Ql, q_stride, 1, g, sp, tw, ktab, kmsum, blk, nb);
    else k_cols_body<LOG2N, MODE, false>(G, g_stride, Gprev, Ql, q_stride, 1, g, sp, tw, ktab, kmsum, blk, nb);
}

// K2's per-bin tables of every column in LDS slot order ([N/2+1][k2_tab_slots]):
// the frame-invariant bin_static values (pyramid masks pre-scaled by inv_nn, a
// power of two: exact), evaluated once per parameter set on the launch stream
// (mm_api.hip launch_k2) instead of in every k_cols workgroup's prologue.
template <int LOG2N, int MODE>
__global__ __launch_bounds__(256) void k_k2_table(float2 *__restrict__ ktab, float *__restrict__ kmsum, Spec sp)
{
    constexpr int N = 1 << LOG2N, TE = k2_tab_entries<LOG2N>(), TS = k2_tab_slots<LOG2N>();
    constexpr int C = fft_c_v(LOG2N), QN = k2_tab_q<LOG2N>();
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= (N / 2 + 1) * TS) return;
    const int f = id / TS, slot = id - f * TS;
    const int e = C == 1 ? slot : (slot % QN) * C + slot / QN;   // k2_tix(e) == slot
    float2 v = make_float2(0.0f, 0.0f);
    float ms = 0.0f;
    if (e < TE) {
        const float ks = k2_tabled<MODE>() ? sp.inv_nn : 1.0f;
        const float2 b = bin_static<LOG2N, MODE>(f, e, sp);
        v = make_float2(b.x * ks, b.y * ks);
        if constexpr (k2_tabled<MODE>()) ms = bin_mask_sum<LOG2N>(f, e, sp) * ks;   // (read by MM_K2_PYR_TAB2)
    }
    ktab[id] = v;
    if constexpr (k2_tabled<MODE>()) kmsum[id] = ms;
}

// =========================================================================
// K3a: row C2R IFFT -> |z| -> horizontal blur -> Yh rows (fp32, global)
// =========================================================================
// One FFT group per pair of Q list rows (ka, ka+1); list row k is canvas row
// (rb + k) mod N.  PerformIFFT (.cs:563-620) ends in |z| (FFT.compute:143-150);
// the horizontal half of ApplyAntiAliasing (.cs:428-429) follows.
// One workgroup per Q tile (TK rows = GPW row pairs; pairs_per_frame = Hq/2
// counts the tile padding, pairs at or past Hn/2 compute but store nothing).
template <int LOG2N>
__global__ __launch_bounds__(k3_threads<LOG2N>())
void k_rows_inv(const c2 *__restrict__ Q, size_t q_stride, float *__restrict__ Yh,
                size_t yh_stride, int frame0, int pairs_per_frame, int total_pairs, Geo g,
                Blur5 bw, const c2 *__restrict__ tw)
{
    constexpr int N = 1 << LOG2N, T = fft_T<LOG2N>(), GPW = k3_groups<LOG2N>(), TK = q_tile<LOG2N>();
    extern __shared__ __attribute__((aligned(16))) c2 lds_all[];
    const int grp = GPW == 1 ? 0 : (T % 64 == 0 ? __builtin_amdgcn_readfirstlane(threadIdx.x / T)
                                               : threadIdx.x / T);
    const int t = GPW == 1 ? threadIdx.x : threadIdx.x % T;
    c2 *lds = lds_all + grp * lds_complex<N>();
    const int logical = xcd_remap(blockIdx.x, gridDim.x) * GPW + grp;
    const int pair = logical % pairs_per_frame;
    const bool valid = logical < total_pairs && 2 * pair < g.Hn;
    const int frame = frame0 + (logical < total_pairs ? logical / pairs_per_frame : 0);
    const int ka = 2 * pair;
    // rows (ka, ka+1) of tile ka / TK: one 16-B piece per bin, TK*8 bytes apart
    // across the wave; the workgroup's groups read the whole TK*8-byte blocks
    const float4 *Qp = reinterpret_cast<const float4 *>(
        Q + (size_t)frame * q_stride + (size_t)(ka / TK) * g.Qs * TK + (ka % TK));
    float4 qv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {   // all 8 loads in flight (addresses always valid)
        const int fq = t + j * T;
        const int ff = fq > N / 2 ? N - fq : fq;
        qv[j] = Qp[(size_t)ff * (TK / 2)];
    }
    c2 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int fq = t + j * T;
        const bool mirror = fq > N / 2;
        const int ff = mirror ? N - fq : fq;
        float4 q = qv[j];
        if (ff == 0 || ff == N / 2) { q.y = 0.0f; q.w = 0.0f; }   // C2R: DC/Nyquist real
        if (mirror) { q.y = -q.y; q.w = -q.w; }                   // X[N-f] = conj X[f]
        v[j] = valid ? mk(q.x - q.w, q.y + q.z) : mk(0.0f, 0.0f); // Z = Qa + i Qb
    }
    fft_regs<LOG2N, +1>(v, t, lds, tw);
    // the four-wide path reads the |z| rows kZShift floats in (taps c-2 .. c+5
    // as two aligned ds_read_b128, see k_rows_inv_compose)
    const bool wide = g.x0 >= 4 && g.x0 % 4 == 0 && g.Wy % 4 == 0 && g.x0 + g.Wy + 4 <= N;
    float *raw = reinterpret_cast<float *>(lds) + (wide ? kZShift : 0);   // [2][N] |z| of rows a, b
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        raw[t + j * T] = fabsf(v[j].x);
        raw[N + t + j * T] = fabsf(v[j].y);
    }
    __syncthreads();
    if (!valid) return;
    float *out = Yh + (size_t)frame * yh_stride + (size_t)ka * g.Wy;
    if (wide) {
        // four outputs per thread, one 16-B store; same expression and order
        // as the scalar form below
        const int W4 = g.Wy / 4;
        const float4 *raw4 = reinterpret_cast<const float4 *>(lds);
        for (int e = t; e < 2 * W4; e += T) {
            const int r = e >= W4 ? 1 : 0, X = 4 * (e - r * W4);
            const float4 *rw = raw4 + ((r * N + g.x0 + X) >> 2);
            const float4 P = rw[0], Z = rw[1];   // z[c-2 .. c+1], z[c+2 .. c+5]
            float4 o;
            o.x = bw.w0 * P.z + bw.w1 * (P.y + P.w) + bw.w2 * (P.x + Z.x);
            o.y = bw.w0 * P.w + bw.w1 * (P.z + Z.x) + bw.w2 * (P.y + Z.y);
            o.z = bw.w0 * Z.x + bw.w1 * (P.w + Z.y) + bw.w2 * (P.z + Z.z);
            o.w = bw.w0 * Z.y + bw.w1 * (Z.x + Z.z) + bw.w2 * (P.w + Z.w);
            st_stream<float4>(out, (unsigned)((r * g.Wy + X) * 4), o);
        }
        return;
    }
    // Wy = W columns (W + 1 for odd W: the crop's second texel)
    const bool interior = g.x0 >= 2 && g.x0 + g.Wy + 2 <= N;
    for (int e = t; e < 2 * g.Wy; e += T) {
        const int r = e >= g.Wy ? 1 : 0, X = e - r * g.Wy;
        const float *rw = raw + r * N;
        const int c = g.x0 + X;
        float acc;
        if (interior) {
            acc = bw.w0 * rw[c] + bw.w1 * (rw[c - 1] + rw[c + 1]) + bw.w2 * (rw[c - 2] + rw[c + 2]);
        } else {
            acc = bw.w0 * rw[wrap_idx(c, N, g.edge)];
            acc += bw.w1 * (rw[wrap_idx(c - 1, N, g.edge)] + rw[wrap_idx(c + 1, N, g.edge)]);
            acc += bw.w2 * (rw[wrap_idx(c - 2, N, g.edge)] + rw[wrap_idx(c + 2, N, g.edge)]);
        }
        out[(size_t)r * g.Wy + X] = acc;
    }
}

// =========================================================================
// K4: vertical blur -> YIQ recombine -> YIQ->RGB -> saturate -> crop
// =========================================================================
// One work-group per tile of kTileRows output rows x kTileCols columns, one
// column per thread: the vertical half of ApplyAntiAliasing (.cs:430-431) on
// Yh, CombineYIQChannels (.cs:437-442; I/Q of the windowed, padded current frame
// re-derived from the input through the same composite resample as K1), the
// YIQ->RGB blit (.cs:200-204) and CropTexture (.cs:386-410).
// The composite taps of image row/column i lie in {i-1, i, i+1} (checked on the
// host), so they are merged into 3 weights (w3 tables) and a tile needs source
// rows [i0-1, i0+TR] x columns [c0-1, c0+TC]: their I/Q are staged once in LDS;
// the horizontal 3-tap combine of every staged row and the TR+4 Yh values of the
// thread's column then live in registers.  One barrier per tile.
#ifndef MM_K4_ROWS
#define MM_K4_ROWS 6   // one-frame calls at 1080p: 8 -> 6 rows per tile 48.4-48.9 -> 47.6-47.8 us per call (4: 49.0-49.2, 16: 49.1-49.8; profiles/r03k_k4_rows_ab.txt)
#endif
#ifndef MM_K4_COLS
#define MM_K4_COLS 256
#endif
constexpr int kTileRows = MM_K4_ROWS, kTileCols = MM_K4_COLS;
// v210's column tile: whole groups of 6 pixels (a tile that split a group would
// split a dword between workgroups), three waves.  The instance is launched
// with that many threads (k4_tile_cols; the launch bound is the larger tile's).
constexpr int kTileColsG = 192;
static_assert(kTileColsG <= kTileCols, "k_compose's launch bound is kTileCols: the group tile must fit it");
template <int FMT> constexpr int k4_tile_cols = kV210<kFmtOut<FMT>> ? kTileColsG : kTileCols;
template <int FMT>
__global__ __launch_bounds__(kTileCols)
void k_compose(const float *__restrict__ Yh, size_t yh_stride, const uint8_t *__restrict__ frames_in,
               uint8_t *__restrict__ frames_out, int frame0, int row_tiles,
               int col_tiles, Geo g, Blur5 bw, const float4 *__restrict__ colW3,
               const float4 *__restrict__ rowW3)
{
    constexpr int TR = kTileRows, TC = k4_tile_cols<FMT>, WC = TC + 2;
    constexpr int FI = kFmtIn<FMT>, FO = kFmtOut<FMT>;   // (a plain format: both are FMT)
    static_assert(kFmtPairOk<FMT>, "a format, or one of the three mixed pairs");
    __shared__ c2 iq[(TR + 2) * WC];         // I/Q of the staged source pixels
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    const int ct = b % col_tiles;
    b /= col_tiles;
    const int rt = b % row_tiles;
    const int frame = frame0 + b / row_tiles;
    const int i0 = rt * TR, c0 = ct * TC;
    const uint8_t *img = frames_in + (size_t)frame * g.li.stride;

    // Staged entry (sr, j) is source pixel (row i0-1+sr, column c0-1+j), wrapped
    // or clamped like the resample's sampler.  Rows are workgroup-uniform (scalar
    // base pointers); thread tid stages column j = tid of every row, and threads
    // 0, 1 also the halo columns j = TC, TC+1.
    using raw_t = typename ChromaSrc<FI>::raw_t;
    // 32-bit offsets from workgroup-uniform row pointers: scalar base + vector
    // offset addressing, no 64-bit address math per access
    // (NV12: the pixel's (Cb, Cr) pair, shared with its 2x2 neighbours)
    auto src_off = [&](int row, unsigned col) {
        if constexpr (k420<FI>) return c420_off<FI>(g, row, col);
        else if constexpr (k422<FI>) return c422_off(g, row, col);
        else if constexpr (kY210<FI>) return y210_off(g, row, col);
        else if constexpr (kV210<FI>) return (unsigned)row * g.li.pitch + v210_pair_off(col);
        else if constexpr (kRGB24<FI>) return (unsigned)row * g.li.pitch;   // (the row: rgb24_px adds the column)
        else return (unsigned)row * g.li.pitch + col * Pix<FI>::bpp;
    };
    // (packed RGB: the byte-aligned dword of the pixel)
    // (v210: the pair's two dwords, its chroma extracted as P010's word pair)
    auto ld_src = [&](int row, unsigned col) {
        if constexpr (kRGB24<FI>) return rgb24_px(img, src_off(row, col), col, g);
        else if constexpr (kV210<FI>) return (raw_t)v210_cword(ld_pair_a4(img, src_off(row, col)), col);
        else if constexpr (kPlanes3<FI>) return (raw_t)c420_pair<FI>(img, g, row, col);   // (a sample of each chroma plane)
        else return ld_off<raw_t>(img, src_off(row, col));
    };
    const unsigned colA = (unsigned)wrap_near(min(c0 - 1 + tid, g.W), g.W, g.edge);
    raw_t pa[TR + 2];
#pragma unroll
    for (int sr = 0; sr < TR + 2; ++sr) {   // all staging loads in flight, then convert
        const int row = wrap_near(min(i0 - 1 + sr, g.H), g.H, g.edge);
        pa[sr] = ld_src(row, colA);
    }
    const int X = c0 + tid;
    const bool vx = X < g.W;
    const float4 wc = colW3[min(X, g.W - 1)];
    // Yh of this column for the TR+4 canvas rows y0+i0-2 .. y0+i0+TR+1 (wrapped
    // or clamped like the blur's sampler, then mapped to Yh list rows), issued
    // before the I/Q conversions so that all loads share one memory round trip
    const float *Yf = Yh + (size_t)frame * yh_stride;
    const unsigned Xc = (unsigned)min(X, g.W - 1);
    float yv[TR + 4];
#pragma unroll
    for (int v = 0; v < TR + 4; ++v) {   // unconditional loads at clamped addresses
        const int cy = wrap_near(g.y0 + i0 - 2 + v, g.N, g.edge);
        const int k = (cy - g.rb + 2 * g.N) & (g.N - 1);
        const float y = ld_off<float>(Yf, (unsigned)(min(k, g.Hn - 1) * g.Wy + Xc) * 4u);
        yv[v] = k < g.Hn ? y : 0.0f;
    }
    // halo columns j = TC, TC + 1 of the TR + 2 rows: one entry for each of
    // threads 0 .. 2(TR+2)-1, loaded with the others (unconditional, clamped)
    constexpr int NH = 2 * (TR + 2);
    const int hs = min(tid, NH - 1);
    const int hrow = wrap_near(min(i0 - 1 + (hs >> 1), g.H), g.H, g.edge);
    const int hcol = wrap_near(min(c0 - 1 + TC + (hs & 1), g.W), g.W, g.edge);
    const raw_t ph = ld_src(hrow, (unsigned)hcol);
    if (tid < NH) iq[(hs >> 1) * WC + TC + (hs & 1)] = src_iq2<FI>(ph, g);
#pragma unroll
    for (int sr = 0; sr < TR + 2; ++sr) iq[sr * WC + tid] = src_iq2<FI>(pa[sr], g);
    __syncthreads();
    // (v210: every lane stays for the barrier of the code exchange below; a lane
    // past W computes from clamped addresses and its codes are not used)
    if constexpr (!kV210<FO>) if (!vx) return;
    [[maybe_unused]] unsigned vcode[kV210<FO> ? TR : 1] = {};   // v210: the rows' codes Y | C << 16
    c2 hc[TR + 2];   // horizontally combined (I, Q) of each staged row
#pragma unroll
    for (int sr = 0; sr < TR + 2; ++sr) {
        const c2 a = iq[sr * WC + tid], m = iq[sr * WC + tid + 1], c = iq[sr * WC + tid + 2];
        hc[sr] = wc.x * a + wc.y * m + wc.z * c;
    }
    uint8_t *outp = frames_out + (size_t)frame * g.lo.stride;
    const VBlur bv = vblur_w<FO>(bw);   // (RGBA8 out: Y' in code units)
    [[maybe_unused]] c2 cd0;   // NV12: the even row's chroma differences
#pragma unroll
    for (int r = 0; r < TR; ++r) {
        const int i = i0 + r;
        if (i < g.H) {
            const float4 wr = rowW3[i];                        // source rows i-1, i, i+1
            const c2 cc = wr.x * hc[r] + wr.y * hc[r + 1] + wr.z * hc[r + 2];   // (ci, cq)
            const float yb = bv.w0 * yv[r + 2] + bv.w1 * (yv[r + 1] + yv[r + 3]) +
                             bv.w2 * (yv[r] + yv[r + 4]);
            [[maybe_unused]] float rr, gg, bb;
            if constexpr (!kCodeOut<FO>) yiq_rgb(yb, cc, rr, gg, bb);
            if constexpr (kRGB24<FO>) {   // three bytes per lane, of the RGBA8 word
                rgb24_store_px(outp + (size_t)((unsigned)i * g.lo.pitch), (unsigned)X, yiq_rgba8(yb, cc), g);
            } else if constexpr (kCodeOut<FO>) {   // one dword per lane, packed in code units
                st_stream<uint32_t>(outp + (unsigned)i * g.lo.pitch, (unsigned)X * 4u, yiq_rgba8<FO>(yb, cc));
            } else if constexpr (k420<FO>) {
                // One luma byte per pixel.  The 2x2 chroma mean: this column's
                // two rows (i0 and TR even: r even starts a block; H even: both
                // rows are inside), plus the neighbour column's from the lane
                // pair (X ^ 1 is tid ^ 1: c0 is even, and W even keeps both
                // lanes past the vx test), exchanged with a quad-perm DPP move.
                // The even lane stores the block's Cb, the odd lane its Cr:
                // byte X of the chroma row.
                static_assert(TR % 2 == 0 && TC % 2 == 0, "NV12: tiles of whole 2x2 blocks");
                c2 cd;
                const unsigned yc = nv12_ycode(rr, gg, bb, g, cd);
                if constexpr (kP010<FO>) {   // one 16-bit word per lane (always aligned)
                    st_off<uint16_t>(outp, (unsigned)i * g.lo.pitch + (unsigned)X * 2u, (uint16_t)(yc << 6));
                } else if constexpr (kI010<FO>) {   // (the code in the word's low bits)
                    st_off<uint16_t>(outp, (unsigned)i * g.lo.pitch + (unsigned)X * 2u, (uint16_t)yc);
                } else {
                    st_off<uint8_t>(outp, (unsigned)i * g.lo.pitch + (unsigned)X, (uint8_t)yc);
                }
                if (r % 2 == 0) {
                    cd0 = cd;
                } else {
                    const c2 v = cd0 + cd;
                    // each lane keeps the component it stores and sends the other one
                    const float mine = X & 1 ? v.y : v.x, send = X & 1 ? v.x : v.y;
                    const float theirs = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(
                        __builtin_bit_cast(int, send), 0xB1, 0xF, 0xF, true));   // quad_perm [1, 0, 3, 2]
                    if constexpr (kP010<FO>) {
                        const unsigned cc10 = p010_ccode(mine + theirs, X & 1 ? g.nv.cro : g.nv.cbo);
                        st_off<uint16_t>(outp, g.lo.c_off + (unsigned)(i >> 1) * g.lo.c_pitch + (unsigned)X * 2u,
                                         (uint16_t)(cc10 << 6));
                    } else if constexpr (kI010<FO>) {
                        // (three planes of words: the even lane's Cb is word X / 2
                        // of the Cb row, the odd lane's Cr the same word of the Cr row)
                        const unsigned cc10 = p010_ccode(mine + theirs, X & 1 ? g.nv.cro : g.nv.cbo);
                        const unsigned co = ((unsigned)X & ~1u) + (X & 1 ? i420_cr_delta(g.lo, g) : 0u);
                        st_off<uint16_t>(outp, g.lo.c_off + (unsigned)(i >> 1) * g.lo.c_pitch + co, (uint16_t)cc10);
                    } else {
                        const unsigned cc8 = nv12_ccode(mine + theirs, X & 1 ? g.nv.cro : g.nv.cbo);
                        // (three planes: the even lane's Cb is byte X / 2 of the
                        // Cb row, the odd lane's Cr the same byte of the Cr row)
                        const unsigned co = kI420<FO> ? ((unsigned)X >> 1) + (X & 1 ? i420_cr_delta(g.lo, g) : 0u) : (unsigned)X;
                        st_off<uint8_t>(outp, g.lo.c_off + (unsigned)(i >> 1) * g.lo.c_pitch + co, (uint8_t)cc8);
                    }
                }
            } else if constexpr (k422<FO>) {
                // The lane pair (X ^ 1 is tid ^ 1: c0 and W are even, as above)
                // is one macropixel.  As for NV12, each lane keeps the chroma
                // component it encodes (even: Cb, odd: Cr) and sends the other
                // one (a quad-perm DPP move): left + right either way.  Its
                // luma and chroma codes are one 16-bit half of the macropixel;
                // the odd lane's half goes to the even lane (a second move),
                // which stores the whole dword.  The odd lane stores nothing.
                static_assert(TC % 2 == 0, "packed 4:2:2: tiles of whole macropixels");
                c2 cd;
                const unsigned yc = nv12_ycode(rr, gg, bb, g, cd);
                const float mine = X & 1 ? cd.y : cd.x, send = X & 1 ? cd.x : cd.y;
                const float theirs = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(
                    __builtin_bit_cast(int, send), 0xB1, 0xF, 0xF, true));   // quad_perm [1, 0, 3, 2]
                const unsigned cc = nv12_ccode(mine + theirs, X & 1 ? g.nv.cro : g.nv.cbo);
                const unsigned half = yc << (8u * g.lo.yb) | cc << (8u - 8u * g.lo.yb);
                const unsigned other = (unsigned)__builtin_amdgcn_mov_dpp((int)half, 0xB1, 0xF, 0xF, true);
                if (!(X & 1))
                    st_stream<uint32_t>(outp + (size_t)((unsigned)i * g.lo.pitch), (unsigned)X * 2u, half | other << 16);
            } else if constexpr (kY210<FO>) {
                // The same exchange with 10-bit codes: a lane's luma and chroma
                // words are one dword of the macropixel, and the even lane
                // stores the macropixel's two dwords (8 bytes, always aligned).
                static_assert(TC % 2 == 0, "packed 4:2:2: tiles of whole macropixels");
                c2 cd;
                const unsigned yc = nv12_ycode(rr, gg, bb, g, cd);
                const float mine = X & 1 ? cd.y : cd.x, send = X & 1 ? cd.x : cd.y;
                const float theirs = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(
                    __builtin_bit_cast(int, send), 0xB1, 0xF, 0xF, true));   // quad_perm [1, 0, 3, 2]
                const unsigned half = y210_half(yc, mine + theirs, X & 1 ? g.nv.cro : g.nv.cbo);
                const unsigned other = (unsigned)__builtin_amdgcn_mov_dpp((int)half, 0xB1, 0xF, 0xF, true);
                if (!(X & 1))
                    st_stream<uint2>(outp + (size_t)((unsigned)i * g.lo.pitch), (unsigned)X * 4u, make_uint2(half, other));
            } else if constexpr (kV210<FO>) {
                // The Y210 branch's codes: the lane pair's chroma sum by the
                // same exchange (c0, a multiple of 6, and W are even), the lane
                // keeps its luma code and the pair's Cb (even) or Cr (odd) code
                // for the group exchange after the row loop.
                static_assert(TC % 6 == 0, "v210: tiles of whole groups");
                c2 cd;
                const unsigned yc = nv12_ycode(rr, gg, bb, g, cd);
                const float mine = X & 1 ? cd.y : cd.x, send = X & 1 ? cd.x : cd.y;
                const float theirs = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(
                    __builtin_bit_cast(int, send), 0xB1, 0xF, 0xF, true));   // quad_perm [1, 0, 3, 2]
                vcode[r] = yc | p010_ccode(mine + theirs, X & 1 ? g.nv.cro : g.nv.cbo) << 16;
            } else {
                Pix<FO>::store(outp + (unsigned)i * g.lo.pitch, (unsigned)X, rr, gg, bb);
            }
        }
    }
    if constexpr (kV210<FO>) {
        // A dword of a group mixes the codes of up to three lanes, and a group's
        // six lanes may lie in two waves (64 is no multiple of 6): the tile's
        // codes go through LDS (over the staged (I, Q), which every lane has
        // read: the barrier in between), and the first lane of each group reads
        // its group's six and stores it whole.  Codes of columns past W are
        // zero: the unused fields of a partial last group.
        static_assert(sizeof(iq) >= sizeof(unsigned) * TR * TC, "the codes fit the staging area");
        unsigned *codes = reinterpret_cast<unsigned *>(iq);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < TR; ++r) codes[r * TC + tid] = vx ? vcode[r] : 0u;
        __syncthreads();
        const unsigned grp = v210_group((unsigned)tid);
        if ((unsigned)tid == 6u * grp && vx) {
            const int n = min(6, g.W - X);
            const unsigned og = v210_group((unsigned)X);
#pragma unroll
            for (int r = 0; r < TR; ++r) {
                const int i = i0 + r;
                if (i < g.H) {
                    unsigned e[6];
#pragma unroll
                    for (int k = 0; k < 6; ++k) e[k] = codes[r * TC + tid + k];
                    v210_store_group(outp + (size_t)((unsigned)i * g.lo.pitch), og, e, n);
                }
            }
        }
    }
}

// k_compose for the single-plane formats (FMT = kFmtY8 / kFmtY16): the same
// tiles, the same Yh loads and the same vertical blur expression, and nothing
// else: (I, Q) of a gray frame is zero, so no input pixel is staged (frames_in
// and the resample tables are not read, no LDS, no barrier) and the pixel is
// the code of sat(Y'), one sample per lane.  Same parameter list as k_compose
// (launch_k4 launches either).
template <int FMT>
__global__ __launch_bounds__(kTileCols)
void k_compose_mono(const float *__restrict__ Yh, size_t yh_stride, const uint8_t *__restrict__,
                    uint8_t *__restrict__ frames_out, int frame0, int row_tiles,
                    int col_tiles, Geo g, Blur5 bw, const float4 *__restrict__,
                    const float4 *__restrict__)
{
    static_assert(kMono<FMT>, "the 4:2:0 and RGBA formats compose with k_compose");
    constexpr int TR = kTileRows, TC = kTileCols;
    int b = blockIdx.x;
    const int ct = b % col_tiles;
    b /= col_tiles;
    const int rt = b % row_tiles;
    const int frame = frame0 + b / row_tiles;
    const int i0 = rt * TR, X = ct * TC + (int)threadIdx.x;
    if (X >= g.W) return;
    const float *Yf = Yh + (size_t)frame * yh_stride;
    float yv[TR + 4];   // canvas rows y0+i0-2 .. y0+i0+TR+1 of this column (k_compose's)
#pragma unroll
    for (int v = 0; v < TR + 4; ++v) {
        const int cy = wrap_near(g.y0 + i0 - 2 + v, g.N, g.edge);
        const int k = (cy - g.rb + 2 * g.N) & (g.N - 1);
        const float y = ld_off<float>(Yf, (unsigned)(min(k, g.Hn - 1) * g.Wy + X) * 4u);
        yv[v] = k < g.Hn ? y : 0.0f;
    }
    uint8_t *outp = frames_out + (size_t)frame * g.lo.stride;
#pragma unroll
    for (int r = 0; r < TR; ++r) {
        const int i = i0 + r;
        if (i < g.H) {
            const float yb = bw.w0 * yv[r + 2] + bw.w1 * (yv[r + 1] + yv[r + 3]) +
                             bw.w2 * (yv[r] + yv[r + 4]);
            mono_store<FMT>(outp + (size_t)((unsigned)i * g.lo.pitch), (unsigned)X, sat(yb), g);
        }
    }
}

// =========================================================================
// K34: K3 + K4 fused (even W, H with W % 8 == 0, N - W >= 8, N - H >= 4)
// =========================================================================
// One workgroup of two FFT groups (2T = N/4 threads >= W/4 column quads) walks
// a strip of R = 4 (steps - 1) output rows of one frame top to bottom.  Step s
// inverse-transforms the Q list-row pairs i0/2 + 2s + {0, 1} (list rows
// i0+4s .. i0+4s+3) exactly as k_rows_inv does, blurs them horizontally from
// LDS, and thread q keeps the blurred values of its quad X = 4q .. 4q+3 in
// registers.  Output row i reads list rows i .. i+4 (rb = y0 - 2 and no row of
// the vertical blur wraps when N - H >= 4), so from step 1 on the 8 list rows
// in registers are the taps of output rows i0+4s-4 .. i0+4s-1, composed as
// k_compose does (same expressions).  Yh never goes through HBM: the frame
// saves its write and re-read (2 x 4 Hn W bytes); a strip re-transforms 4
// halo rows (4 / R more Q reads and FFT work).
#ifdef MM_K34_STAMPS
// Diagnostic build only: per-wave cycle totals of the strip-step phases
// (s_memtime deltas), written by lane 0 with a vector store after the walk.
__device__ unsigned long long mm_k34_stamps[65536 * 8];
#define K34_STAMP(i)                                                     \
    do {                                                                 \
        const unsigned long long n_ = __builtin_amdgcn_s_memtime();      \
        st_acc[i] += n_ - st_prev;                                       \
        st_prev = n_;                                                    \
    } while (0)
#else
#define K34_STAMP(i) do { } while (0)
#endif
// SRCDMA (4-byte pixels, every source row of the launch on a multiple of 16
// bytes: launch_k3): the compose's four new source rows per step do not go
// through registers.  Each thread copies its quad of each row to LDS with one
// global_load_lds_dwordx4 (no VGPR destination), issued between pass 0 and
// pass 1 of the step's inverse FFT, so the round trip to memory runs under the
// rest of the transform and the blur instead of in front of the compose; the
// compose reads its six pixels per row from the staged rows.  Four rows of
// 2T x 16 = 4 N bytes IN FRONT of the FFT regions (thread q's piece at 16 q:
// wave base + lane x 16, the only destination form an LDS-DMA has).  A staged
// row is the pixel row itself (pixel x at 4 x: the clamped quads of threads
// past W land behind it), so the neighbour pixels cl / cr, whichever wave
// copied them, are plain indexed reads.  Order: the DMA follows the two
// barriers of pass 0, which every wave reaches only after its previous compose
// (the last reader of the rows); each wave waits for its own copies before the
// barrier that ends the blur, and the compose reads after that barrier.
// (... and the encode pair's, MM_RGBA8 in with NV12 out: the same 4-byte source pixels)
template <int FMT> constexpr bool k34_dma_fmt = FMT == MM_RGBA8 || FMT == MM_RGBA8_SRGB || FMT == kFmtRGBA8toNV12 ||
                                                FMT == kFmtBGRA8 || FMT == kFmtBGRA8S || FMT == kFmtBGRA8toNV12;
template <int LOG2N> constexpr int k34_src_bytes() { return 4 * 4 * (1 << LOG2N); }
template <int LOG2N, int FMT, bool SRCDMA = false>
__global__ __launch_bounds__(2 * fft_T<LOG2N>()) __attribute__((amdgpu_waves_per_eu(4)))
void k_rows_inv_compose(const c2 *__restrict__ Q, size_t q_stride,
                        const uint8_t *__restrict__ frames_in, uint8_t *__restrict__ frames_out,
                        int frame0, int strips, int steps, Geo g, Blur5 bw,
                        const float4 *__restrict__ colW3, const float4 *__restrict__ rowW3,
                        const c2 *__restrict__ tw)
{
    constexpr int N = 1 << LOG2N, T = fft_T<LOG2N>(), TK = q_tile<LOG2N>();
    constexpr int FI = kFmtIn<FMT>, FO = kFmtOut<FMT>;   // (a plain format: both are FMT)
    static_assert(kFmtPairOk<FMT>, "a format, or one of the three mixed pairs");
    using raw_t = typename ChromaSrc<FI>::raw_t;
    constexpr unsigned bpp = LumaSrc<FI>::bpp;   // (NV12: 1, the luma plane's)
    [[maybe_unused]] constexpr unsigned bppo = LumaSrc<FO>::bpp;   // ... and the output side's
    static_assert(!SRCDMA || k34_dma_fmt<FMT>, "staged source rows: 4-byte pixels");
    extern __shared__ __attribute__((aligned(16))) c2 lds_raw[];
    [[maybe_unused]] const uint8_t *srcl = reinterpret_cast<const uint8_t *>(lds_raw);   // [4][4 N] staged rows
    c2 *lds_all = lds_raw + (SRCDMA ? k34_src_bytes<LOG2N>() / (int)sizeof(c2) : 0);
    const int grp = T % 64 == 0 ? __builtin_amdgcn_readfirstlane(threadIdx.x / T) : threadIdx.x / T;
    const int t = threadIdx.x % T;
    c2 *lds = lds_all + grp * lds_complex<N>();
    const float *raw_all = reinterpret_cast<const float *>(lds_all);
    constexpr int GROUP_FLOATS = 2 * lds_complex<N>();
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int frame = frame0 + b / strips;
    const int i0 = (b % strips) * 4 * (steps - 1);
    const c2 *Qf = Q + (size_t)frame * q_stride;
    const uint8_t *img = frames_in + (size_t)frame * g.li.stride;
    uint8_t *outp = frames_out + (size_t)frame * g.lo.stride;

    const int q = threadIdx.x;
    const bool vq = 4 * q < g.W;
    const int X = vq ? 4 * q : g.W - 4;     // clamped quad (loads stay in the image)
    const unsigned cl = (unsigned)wrap_near(X - 1, g.W, g.edge);
    const unsigned cr = (unsigned)wrap_near(X + 4, g.W, g.edge);
    // horizontally combined I/Q of one source row for the quad (k_compose's
    // staged 3-tap combine over columns X-1 .. X+4)
    auto chroma_row = [&](int i, c2 (&hc)[4]) {
        if constexpr (!kMono<FI>) {   // (a gray frame's (I, Q) is zero: nothing to read)
            const int row = wrap_near(min(i, g.H), g.H, g.edge);
            c2 a[6];
            if constexpr (k422<FI>) {
                // macropixels X/2-1 .. X/2+2: the quad's own two as one 8-byte load
                c422_quad_iq(img, g, row, (unsigned)X, cl, cr, a);
            } else if constexpr (kY210<FI>) {
                // ... of 8 bytes each: the quad's own two as one 16-byte load
                y210_quad_iq(img, g, row, (unsigned)X, cl, cr, a);
            } else if constexpr (kRGB24<FI>) {
                // three-byte pixels: the quad's own four as one 12-byte load
                rgb24_quad_iq(img, g, row, (unsigned)X, cl, cr, a);
            } else if constexpr (k420<FI>) {
                // source columns X-1 .. X+4 are chroma samples X/2-1 .. X/2+2 (the
                // outer two wrapped or clamped as pixels, then halved): the quad's
                // own two pairs as one dword (X % 4 == 0, chroma rows dword aligned
                // in every frame of the launch: nv12_quads_aligned), the outer two as 2-byte loads
                // (P010: pairs are dwords, the quad's own two as two dword loads)
                const unsigned pl = c420_pair<FI>(img, g, row, cl);
                unsigned pm0, pm1;
                c420_quad_pairs<FI>(img, g, row, (unsigned)X, pm0, pm1);
                const unsigned pr = c420_pair<FI>(img, g, row, cr);
                a[0] = c420_iq2<FI>(pl, g);
                a[1] = a[2] = c420_iq2<FI>(pm0, g);
                a[3] = a[4] = c420_iq2<FI>(pm1, g);
                a[5] = c420_iq2<FI>(pr, g);
            } else {
                // (in pixels: an RGBA pitch is a multiple of the pixel size)
                const unsigned base = (unsigned)row * (g.li.pitch / bpp);
                raw_t p[6];
                p[0] = ld_off<raw_t>(img, (base + cl) * bpp);
                if constexpr (bpp == 4) {   // one 16-byte load (dword aligned: ld_quad_a4)
                    const uint4 m = ld_quad_a4(img, (base + (unsigned)X) * bpp);
                    p[1] = m.x; p[2] = m.y; p[3] = m.z; p[4] = m.w;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) p[1 + k] = ld_off<raw_t>(img, (base + (unsigned)X + k) * bpp);
                }
                p[5] = ld_off<raw_t>(img, (base + cr) * bpp);
#pragma unroll
                for (int k = 0; k < 6; ++k) a[k] = chroma_iq2<FI>(p[k]);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 wc = colW3[X + k];
                hc[k] = wc.x * a[k] + wc.y * a[k + 1] + wc.z * a[k + 2];
            }
        }
    };
    // SRCDMA: the step's source row r (i0+4s-3+r) to LDS, and chroma_row's
    // RGBA branch on the staged row (the same six pixels, the same expressions)
    [[maybe_unused]] auto stage_row = [&](int i, int r) {
        if constexpr (SRCDMA) {
            typedef __attribute__((address_space(1))) const void gptr_t;
            typedef __attribute__((address_space(3))) void lptr_t;
            // wrap_near(min(i, H), H, edge) for i >= 0 (a staged row is i0 + 1 or later)
            const int row = i < g.H ? i : (g.edge ? g.H - 1 : 0);
            const uint8_t *src = img + (size_t)((unsigned)row * g.li.pitch) + (unsigned)X * 4u;
            // the wave's base (a scalar): the hardware adds lane x 16
            const unsigned wbase = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x & ~63u)) * 16u;
            const uint8_t *dst = srcl + r * (4 * N) + wbase;
            __builtin_amdgcn_global_load_lds((gptr_t *)src, (lptr_t *)dst, 16, 0, 0);
        }
    };
    [[maybe_unused]] auto chroma_row_staged = [&](int r, c2 (&hc)[4]) {
        if constexpr (SRCDMA) {
            const uint8_t *rowp = srcl + r * (4 * N);
            unsigned p[6];
            p[0] = *reinterpret_cast<const unsigned *>(rowp + cl * 4u);
            const uint4 m = *reinterpret_cast<const uint4 *>(rowp + (unsigned)X * 4u);
            p[1] = m.x; p[2] = m.y; p[3] = m.z; p[4] = m.w;
            p[5] = *reinterpret_cast<const unsigned *>(rowp + cr * 4u);
            c2 a[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) a[k] = chroma_iq2<FI>(p[k]);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 wc = colW3[X + k];
                hc[k] = wc.x * a[k] + wc.y * a[k + 1] + wc.z * a[k + 2];
            }
        }
    };

    float yw[8][4];            // list rows i0+4s-4 .. i0+4s+3 of the quad (blurred horizontally)
                               // (as column pairs for a packed vertical blur: +3 spills, not kept)
    [[maybe_unused]] c2 hc[6][4];   // combined (I, Q) of source rows i0+4s-5 .. i0+4s (gray: none)
    [[maybe_unused]] const VBlur bv = vblur_w<FO>(bw);   // the compose's vertical blur (RGBA8 out: in code units)
    chroma_row(i0 - 1, hc[4]);
    chroma_row(i0, hc[5]);
#ifdef MM_K34_STAMPS
    unsigned long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long st_prev = __builtin_amdgcn_s_memtime();
    st_acc[7] = __builtin_amdgcn_s_memrealtime();
#endif
    // Q rows of step s: list-row pair i0/2 + 2s + grp (zero beyond Hn)
    float4 qv[8];
    auto load_q = [&](int s_) {
        const int ka_ = i0 + 4 * s_ + 2 * grp;
        const int kl = ka_ < g.Hn ? ka_ : 0;
        const float4 *Qp = reinterpret_cast<const float4 *>(Qf + (size_t)(kl / TK) * g.Qs * TK + (kl % TK));
        // column ff = t + jT (j < 4) or N - t - jT (j >= 4; = N/2 at t = 0,
        // j = 4): a workgroup-uniform base per j plus one of two per-thread
        // offsets, not eight loop-invariant VGPR offsets
        const unsigned up = (unsigned)t * (TK / 2), dn = (unsigned)(T - 1 - t) * (TK / 2);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j < 4) qv[j] = (Qp + (size_t)(j * T) * (TK / 2))[up];
            else qv[j] = (Qp + (size_t)(N - j * T - (T - 1)) * (TK / 2))[dn];
        }
    };
    for (int s = 0; s < steps; ++s) {
        const int ka = i0 + 4 * s + 2 * grp;
        const bool valid = ka < g.Hn;
        load_q(s);
        c2 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int fq = t + j * T;
            const bool mirror = fq > N / 2;
            const int ff = mirror ? N - fq : fq;
            float4 qq = qv[j];
            if (ff == 0 || ff == N / 2) { qq.y = 0.0f; qq.w = 0.0f; }
            if (mirror) { qq.y = -qq.y; qq.w = -qq.w; }
            v[j] = valid ? mk(qq.x - qq.w, qq.y + qq.z) : mk(0.0f, 0.0f);
        }
        K34_STAMP(0);
        if constexpr (SRCDMA) {
            // fft_regs, with the source rows' copies issued behind pass 0: after
            // the Q loads in program order (their wait does not cover the
            // copies) and after its barriers (the staged rows are free)
            c2 wb[kTwSlots];
            preload_twiddles<LOG2N>(wb, t, tw);
            fft_pass<LOG2N, 0, +1>(v, t, lds, wb);
            if (s > 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) stage_row(i0 + 4 * s - 3 + r, r);
            }
            // (barriers that order LDS only: the copies stay in flight)
            fft_pass_loop<LOG2N, +1, 1, kSyncLds>(v, t, lds, wb);
        } else {
            fft_regs<LOG2N, +1>(v, t, lds, tw);
        }
        K34_STAMP(1);
        float *raw = reinterpret_cast<float *>(lds) + kZShift;   // [2][N] |z| of rows ka, ka+1
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            raw[t + j * T] = fabsf(v[j].x);
            raw[N + t + j * T] = fabsf(v[j].y);
        }
        xsync<SRCDMA ? kSyncLds : 0>();
        K34_STAMP(2);
        // ---- horizontal blur of the 4 new list rows ----
        // |z| rows sit 2 floats into their LDS rows (zshift), so the taps
        // c-2 .. c+5 of the quad are TWO 16-B aligned ds_read_b128 (conflict-
        // free: consecutive 16 B per lane) instead of the compiler's two
        // ds_read2_b64 of 8-B aligned halves (2-way conflicts on every one,
        // tools/lds_banks.py "k34"); same expressions and order as k_rows_inv
        // one base address; the rows are immediate offsets
        const float4 *b4 = reinterpret_cast<const float4 *>(raw_all) + ((g.x0 + X) >> 2);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float4 *r4 = b4 + ((r >> 1) * GROUP_FLOATS + (r & 1) * N) / 4;
            float4 P, Z;   // z[c-2 .. c+1], z[c+2 .. c+5]
            if constexpr (SRCDMA) {
                // (read as lds_ld reads: the compiler then orders these reads
                // of the FFT regions behind no copy into the staged rows)
                typedef float f32x4 __attribute__((ext_vector_type(4)));
                typedef __attribute__((address_space(3))) const volatile f32x4 lds_vf4;
                const f32x4 p = *(lds_vf4 *)(r4), z = *(lds_vf4 *)(r4 + 1);
                P = make_float4(p.x, p.y, p.z, p.w);
                Z = make_float4(z.x, z.y, z.z, z.w);
            } else {
                P = r4[0];
                Z = r4[1];
            }
            yw[4 + r][0] = bw.w0 * P.z + bw.w1 * (P.y + P.w) + bw.w2 * (P.x + Z.x);
            yw[4 + r][1] = bw.w0 * P.w + bw.w1 * (P.z + Z.x) + bw.w2 * (P.y + Z.y);
            yw[4 + r][2] = bw.w0 * Z.x + bw.w1 * (P.w + Z.y) + bw.w2 * (P.z + Z.z);
            yw[4 + r][3] = bw.w0 * Z.y + bw.w1 * (Z.x + Z.z) + bw.w2 * (P.w + Z.w);
        }
        // (SRCDMA: the wave's own copies have landed before it arrives)
        if constexpr (SRCDMA) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();   // LDS free for the next step's FFT
        K34_STAMP(3);
        if (s > 0) {
            // ---- K4 on output rows i0+4s-4 .. i0+4s-1, two at a time ----
            // the 4 chroma rows' loads first (one memory round trip)
            if constexpr (k420<FI>) {
                // source rows 2j and 2j+1 share a chroma row (i0 % 4 == 0, H
                // even): row i0+4s-3 has the kept row i0+4s-4's samples, row
                // i0+4s-1 those of i0+4s-2; two loads per step, not four
#pragma unroll
                for (int k = 0; k < 4; ++k) hc[2][k] = hc[1][k];
                chroma_row(i0 + 4 * s - 2, hc[3]);
#pragma unroll
                for (int k = 0; k < 4; ++k) hc[4][k] = hc[3][k];
                chroma_row(i0 + 4 * s, hc[5]);
            } else if constexpr (SRCDMA) {
#pragma unroll
                for (int r = 0; r < 4; ++r) chroma_row_staged(r, hc[2 + r]);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) chroma_row(i0 + 4 * s - 3 + r, hc[2 + r]);
            }
            [[maybe_unused]] c2 cd0[4];   // NV12: the even row's chroma differences
            for (int r = 0; r < 4; ++r) {
                K34_STAMP(4);
                const int i = i0 + 4 * s - 4 + r;
                if constexpr (kMono<FMT>) {
                    // a gray frame: the code of sat(Y'), the blur written as below
                    if (vq && i < g.H) {
                        float yl[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const float yb = bw.w0 * yw[r + 2][k] + bw.w1 * (yw[r + 1][k] + yw[r + 3][k]) +
                                             bw.w2 * (yw[r][k] + yw[r + 4][k]);
                            yl[k] = sat(yb);
                        }
                        mono_store_quad<FMT>(outp + (size_t)((unsigned)i * g.lo.pitch), (unsigned)X, yl, g);
                    }
                } else if (vq && i < g.H) {
                    const float4 wr = rowW3[i];
                    [[maybe_unused]] float rr[4], gg[4], bb[4];
                    [[maybe_unused]] uint32_t pc[4];   // RGBA8 / packed RGB out: the quad's RGBA8 words, packed in code units
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const c2 cc = wr.x * hc[r][k] + wr.y * hc[r + 1][k] + wr.z * hc[r + 2][k];
                        const float yb = bv.w0 * yw[r + 2][k] + bv.w1 * (yw[r + 1][k] + yw[r + 3][k]) +
                                         bv.w2 * (yw[r][k] + yw[r + 4][k]);
                        if constexpr (kCodeOut<FO>) pc[k] = yiq_rgba8<FO>(yb, cc);
                        else yiq_rgb(yb, cc, rr[k], gg[k], bb[k]);
                    }
                    // (in pixels: an RGBA pitch is a multiple of the pixel size)
                    [[maybe_unused]] const unsigned o = (unsigned)i * (g.lo.pitch / bppo) + (unsigned)X;
                    if constexpr (kRGB24<FO>) {
                        rgb24_store_quad(outp, g, i, X, pc);
                    } else if constexpr (kCodeOut<FO>) {
                        // (scalar row base + the thread's column offset, as below)
                        st_stream_quad_a4(outp + (size_t)((unsigned)i * g.lo.pitch), (unsigned)X * 4u,
                                          make_uint4(pc[0], pc[1], pc[2], pc[3]));
                    } else if constexpr (k422<FO>) {
                        c422_store_quad(outp, g, i, X, rr, gg, bb);
                    } else if constexpr (kY210<FO>) {
                        y210_store_quad(outp, g, i, X, rr, gg, bb);
                    } else if constexpr (k420<FO>) {
                        c420_store_quad<FO>(outp, g, i, X, r & 1, rr, gg, bb, cd0);
                    } else if constexpr (bppo == 4) {
                        uint4 px;
                        px.x = Pix<FO>::pack(rr[0], gg[0], bb[0]);
                        px.y = Pix<FO>::pack(rr[1], gg[1], bb[1]);
                        px.z = Pix<FO>::pack(rr[2], gg[2], bb[2]);
                        px.w = Pix<FO>::pack(rr[3], gg[3], bb[3]);
                        // scalar row base + the thread's column offset: one
                        // live VGPR, not a hoisted offset per row
                        st_stream_quad_a4(outp + (size_t)((unsigned)i * g.lo.pitch), (unsigned)X * 4u, px);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k) Pix<FO>::store(outp, o + k, rr[k], gg[k], bb[k]);
                    }
                }
            }
        }
        K34_STAMP(5);
        // ---- slide: keep list rows i0+4s .. +3 and source rows i0+4s-1, i0+4s
        // (after step 0: the primed rows i0-1, i0) ----
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int k = 0; k < 4; ++k) yw[r][k] = yw[4 + r][k];
        if constexpr (!kMono<FMT>) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                hc[0][k] = hc[4][k];
                hc[1][k] = hc[5][k];
            }
        }
    }
#ifdef MM_K34_STAMPS
    st_acc[6] = (unsigned long long)steps;
    st_acc[7] = (__builtin_amdgcn_s_memrealtime() - st_acc[7]) << 32 | (st_acc[7] & 0xffffffffull);
    const int w = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    if (threadIdx.x % 64 == 0 && w < 65536)
        for (int i = 0; i < 8; ++i) mm_k34_stamps[w * 8 + i] = st_acc[i];
#endif
}

// K34 in one shot, for short launches (the one-frame drop-in call): a strip of
// 4 output rows needs list rows i0 .. i0+7, so a workgroup of FOUR FFT groups
// transforms all of them at once (group g: list-row pair i0/2 + g, exactly
// k_rows_inv_compose's step code), and then its two halves compose output
// rows i0 + 2hh and i0 + 2hh + 1 (hh = 0, 1) from the 6 list rows and 4 source
// rows they read: no sequential walk.  Twice the FFTs of the walking form
// (every list row is transformed by two strips), but one workgroup round, one
// launch instead of K3 + K4, and no Yh round trip.  Same expressions in the
// same order as K3 + K4: bitwise equal (tests/test_k34.py).  N <= 2048 (4T
// threads <= 1024).
template <int LOG2N, int FMT>
__global__ __launch_bounds__(4 * fft_T<LOG2N>())
void k_rows_inv_compose4(const c2 *__restrict__ Q, size_t q_stride,
                         const uint8_t *__restrict__ frames_in, uint8_t *__restrict__ frames_out,
                         int frame0, int strips, Geo g, Blur5 bw,
                         const float4 *__restrict__ colW3, const float4 *__restrict__ rowW3,
                         const c2 *__restrict__ tw)
{
    constexpr int N = 1 << LOG2N, T = fft_T<LOG2N>(), TK = q_tile<LOG2N>();
    constexpr int FI = kFmtIn<FMT>, FO = kFmtOut<FMT>;   // (a plain format: both are FMT)
    static_assert(kFmtPairOk<FMT>, "a format, or one of the three mixed pairs");
    using raw_t = typename ChromaSrc<FI>::raw_t;
    constexpr unsigned bpp = LumaSrc<FI>::bpp;   // (NV12: 1, the luma plane's)
    [[maybe_unused]] constexpr unsigned bppo = LumaSrc<FO>::bpp;   // ... and the output side's
    extern __shared__ __attribute__((aligned(16))) c2 lds_all[];
    const int grp = T % 64 == 0 ? __builtin_amdgcn_readfirstlane(threadIdx.x / T) : threadIdx.x / T;
    const int t = threadIdx.x % T;
    c2 *lds = lds_all + grp * lds_complex<N>();
    const float *raw_all = reinterpret_cast<const float *>(lds_all);
    constexpr int GROUP_FLOATS = 2 * lds_complex<N>();
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int frame = frame0 + b / strips;
    const int i0 = (b % strips) * 4;
    const c2 *Qf = Q + (size_t)frame * q_stride;
    const uint8_t *img = frames_in + (size_t)frame * g.li.stride;
    uint8_t *outp = frames_out + (size_t)frame * g.lo.stride;

    // ---- K3 on list-row pair i0/2 + grp (zero beyond Hn) ----
    {
        const int ka = i0 + 2 * grp;
        const bool valid = ka < g.Hn;
        const int kl = valid ? ka : 0;
        const float4 *Qp = reinterpret_cast<const float4 *>(Qf + (size_t)(kl / TK) * g.Qs * TK + (kl % TK));
        float4 qv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int fq = t + j * T;
            const int ff = fq > N / 2 ? N - fq : fq;
            qv[j] = Qp[(size_t)ff * (TK / 2)];
        }
        c2 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int fq = t + j * T;
            const bool mirror = fq > N / 2;
            const int ff = mirror ? N - fq : fq;
            float4 qq = qv[j];
            if (ff == 0 || ff == N / 2) { qq.y = 0.0f; qq.w = 0.0f; }
            if (mirror) { qq.y = -qq.y; qq.w = -qq.w; }
            v[j] = valid ? mk(qq.x - qq.w, qq.y + qq.z) : mk(0.0f, 0.0f);
        }
        fft_regs<LOG2N, +1>(v, t, lds, tw);
        float *raw = reinterpret_cast<float *>(lds) + kZShift;   // [2][N] |z| of rows ka, ka+1
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            raw[t + j * T] = fabsf(v[j].x);
            raw[N + t + j * T] = fabsf(v[j].y);
        }
    }
    __syncthreads();

    // ---- compose: half hh of the workgroup, output rows i0 + 2hh, i0 + 2hh + 1 ----
    const int q = threadIdx.x % (2 * T), hh = threadIdx.x / (2 * T);
    const bool vq = 4 * q < g.W;
    const int X = vq ? 4 * q : g.W - 4;
    const unsigned cl = (unsigned)wrap_near(X - 1, g.W, g.edge);
    const unsigned cr = (unsigned)wrap_near(X + 4, g.W, g.edge);
    auto chroma_row = [&](int i, c2 (&hc)[4]) {   // k_rows_inv_compose's
        if constexpr (!kMono<FI>) {   // (a gray frame's (I, Q) is zero: nothing to read)
            const int row = wrap_near(min(i, g.H), g.H, g.edge);
            c2 a[6];
            if constexpr (k422<FI>) {
                // macropixels X/2-1 .. X/2+2: the quad's own two as one 8-byte load
                c422_quad_iq(img, g, row, (unsigned)X, cl, cr, a);
            } else if constexpr (kY210<FI>) {
                // ... of 8 bytes each: the quad's own two as one 16-byte load
                y210_quad_iq(img, g, row, (unsigned)X, cl, cr, a);
            } else if constexpr (kRGB24<FI>) {
                // three-byte pixels: the quad's own four as one 12-byte load
                rgb24_quad_iq(img, g, row, (unsigned)X, cl, cr, a);
            } else if constexpr (k420<FI>) {
                // source columns X-1 .. X+4 are chroma samples X/2-1 .. X/2+2 (the
                // outer two wrapped or clamped as pixels, then halved): the quad's
                // own two pairs as one dword (X % 4 == 0, chroma rows dword aligned
                // in every frame of the launch: nv12_quads_aligned), the outer two as 2-byte loads
                // (P010: pairs are dwords, the quad's own two as two dword loads)
                const unsigned pl = c420_pair<FI>(img, g, row, cl);
                unsigned pm0, pm1;
                c420_quad_pairs<FI>(img, g, row, (unsigned)X, pm0, pm1);
                const unsigned pr = c420_pair<FI>(img, g, row, cr);
                a[0] = c420_iq2<FI>(pl, g);
                a[1] = a[2] = c420_iq2<FI>(pm0, g);
                a[3] = a[4] = c420_iq2<FI>(pm1, g);
                a[5] = c420_iq2<FI>(pr, g);
            } else {
                // (in pixels: an RGBA pitch is a multiple of the pixel size)
                const unsigned base = (unsigned)row * (g.li.pitch / bpp);
                raw_t p[6];
                p[0] = ld_off<raw_t>(img, (base + cl) * bpp);
                if constexpr (bpp == 4) {   // one 16-byte load (dword aligned: ld_quad_a4)
                    const uint4 m = ld_quad_a4(img, (base + (unsigned)X) * bpp);
                    p[1] = m.x; p[2] = m.y; p[3] = m.z; p[4] = m.w;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) p[1 + k] = ld_off<raw_t>(img, (base + (unsigned)X + k) * bpp);
                }
                p[5] = ld_off<raw_t>(img, (base + cr) * bpp);
#pragma unroll
                for (int k = 0; k < 6; ++k) a[k] = chroma_iq2<FI>(p[k]);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 wc = colW3[X + k];
                hc[k] = wc.x * a[k] + wc.y * a[k + 1] + wc.z * a[k + 2];
            }
        }
    };
    const int r0 = i0 + 2 * hh;   // first output row of this half
    [[maybe_unused]] c2 hc[4][4];   // combined (I, Q) of source rows r0-1 .. r0+2 (gray: none)
    if constexpr (kMono<FMT>) {
        // (nothing to read)
    } else if constexpr (k420<FI>) {   // rows r0, r0+1 (r0 even) share a chroma row
        chroma_row(r0 - 1, hc[0]);
        chroma_row(r0, hc[1]);
#pragma unroll
        for (int k = 0; k < 4; ++k) hc[2][k] = hc[1][k];
        chroma_row(r0 + 2, hc[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) chroma_row(r0 - 1 + k, hc[k]);
    }
    float yw[6][4];               // list rows r0 .. r0+5 of the quad, blurred horizontally
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int r = 2 * hh + k;   // list row i0 + r: group r/2, row r%2 (zshift: k_rows_inv_compose)
        const float4 *r4 = reinterpret_cast<const float4 *>(raw_all) + ((g.x0 + X) >> 2) +
                           ((r >> 1) * GROUP_FLOATS + (r & 1) * N) / 4;
        const float4 P = r4[0], Z = r4[1];   // z[c-2 .. c+1], z[c+2 .. c+5]
        yw[k][0] = bw.w0 * P.z + bw.w1 * (P.y + P.w) + bw.w2 * (P.x + Z.x);
        yw[k][1] = bw.w0 * P.w + bw.w1 * (P.z + Z.x) + bw.w2 * (P.y + Z.y);
        yw[k][2] = bw.w0 * Z.x + bw.w1 * (P.w + Z.y) + bw.w2 * (P.z + Z.z);
        yw[k][3] = bw.w0 * Z.y + bw.w1 * (Z.x + Z.z) + bw.w2 * (P.w + Z.w);
    }
    [[maybe_unused]] const VBlur bv = vblur_w<FO>(bw);   // the vertical blur (RGBA8 out: in code units)
    [[maybe_unused]] c2 cd0[4];   // NV12: the even row's chroma differences
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int i = r0 + r;
        if constexpr (kMono<FMT>) {   // the code of sat(Y') (k_rows_inv_compose's)
            if (vq && i < g.H) {
                float yl[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float yb = bw.w0 * yw[r + 2][k] + bw.w1 * (yw[r + 1][k] + yw[r + 3][k]) +
                                     bw.w2 * (yw[r][k] + yw[r + 4][k]);
                    yl[k] = sat(yb);
                }
                mono_store_quad<FMT>(outp + (size_t)((unsigned)i * g.lo.pitch), (unsigned)X, yl, g);
            }
        } else if (vq && i < g.H) {
            const float4 wr = rowW3[i];
            [[maybe_unused]] float rr[4], gg[4], bb[4];
            [[maybe_unused]] uint32_t pc[4];   // RGBA8 / packed RGB out: the quad's RGBA8 words, packed in code units
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const c2 cc = wr.x * hc[r][k] + wr.y * hc[r + 1][k] + wr.z * hc[r + 2][k];
                const float yb = bv.w0 * yw[r + 2][k] + bv.w1 * (yw[r + 1][k] + yw[r + 3][k]) +
                                 bv.w2 * (yw[r][k] + yw[r + 4][k]);
                if constexpr (kCodeOut<FO>) pc[k] = yiq_rgba8<FO>(yb, cc);
                else yiq_rgb(yb, cc, rr[k], gg[k], bb[k]);
            }
            [[maybe_unused]] const unsigned o = (unsigned)i * (g.lo.pitch / bppo) + (unsigned)X;
            if constexpr (kRGB24<FO>) {
                rgb24_store_quad(outp, g, i, X, pc);
            } else if constexpr (kCodeOut<FO>) {
                st_stream_quad_a4(outp, o * 4u, make_uint4(pc[0], pc[1], pc[2], pc[3]));
            } else if constexpr (k422<FO>) {
                c422_store_quad(outp, g, i, X, rr, gg, bb);
            } else if constexpr (kY210<FO>) {
                y210_store_quad(outp, g, i, X, rr, gg, bb);
            } else if constexpr (k420<FO>) {
                c420_store_quad<FO>(outp, g, i, X, r & 1, rr, gg, bb, cd0);
            } else if constexpr (bppo == 4) {
                uint4 px;
                px.x = Pix<FO>::pack(rr[0], gg[0], bb[0]);
                px.y = Pix<FO>::pack(rr[1], gg[1], bb[1]);
                px.z = Pix<FO>::pack(rr[2], gg[2], bb[2]);
                px.w = Pix<FO>::pack(rr[3], gg[3], bb[3]);
                st_stream_quad_a4(outp, o * 4u, px);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) Pix<FO>::store(outp, o + k, rr[k], gg[k], bb[k]);
            }
        }
    }
}

// K4 for odd W and/or H: the quad's edge then sits half a texel off the
// texel grid (x0 + 0.5), and CropTexture (.cs:386-410) samples the final
// texture between two texels (four when both are odd) with weights 1/2: output
// pixel (X, Y) = mean of saturate(YIQ->RGB) at canvas texels x0 + X (+1),
// y0 + Y (+1) (oracle mm_ref.c crop).  A texel outside the quad has I = Q = 0
// (the cleared canvas) and the blurred Y' of that position.  One thread per
// output pixel; the I/Q of a texel is the composite resample from the unmerged
// Tap4 tables (taps on i-2 .. i+1 for odd sizes).
template <int FMT>
__global__ __launch_bounds__(256)
void k_compose_odd(const float *__restrict__ Yh, size_t yh_stride, const uint8_t *__restrict__ frames_in,
                   uint8_t *__restrict__ frames_out, int frame0, int nframes, Geo g,
                   Blur5 bw, const Tap4 *__restrict__ colT, const Tap4 *__restrict__ rowT)
{
    const size_t npx = (size_t)g.W * g.H;
    const size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (e >= npx * nframes) return;
    const int k = (int)(e / npx);
    const int p = (int)(e - (size_t)k * npx);
    const int Y = p / g.W, X = p - Y * g.W;
    const int frame = frame0 + k;
    const uint8_t *img = frames_in + (size_t)frame * g.li.stride;
    const float *Yf = Yh + (size_t)frame * yh_stride;
    const float wt = (g.ox ? 0.5f : 1.0f) * (g.oy ? 0.5f : 1.0f);
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int dy = 0; dy <= g.oy; ++dy)
        for (int dx = 0; dx <= g.ox; ++dx) {
            const int tx = X + dx, ty = Y + dy;   // texel's image column / row (may be W / H)
            // Y': vertical 5-tap blur of Yh (list row of canvas row y0+ty+d is ty+2+d)
            float yv[5];
            for (int d = 0; d < 5; ++d) {
                const int cy = wrap_near(g.y0 + ty - 2 + d, g.N, g.edge);
                const int kk = (cy - g.rb + 2 * g.N) & (g.N - 1);
                yv[d] = kk < g.Hn ? Yf[(size_t)kk * g.Wy + tx] : 0.0f;
            }
            const float yb = bw.w0 * yv[2] + bw.w1 * (yv[1] + yv[3]) + bw.w2 * (yv[0] + yv[4]);
            float ci = 0.0f, cq = 0.0f;
            // (a gray frame's (I, Q) is zero: its instances read no input pixel)
            if constexpr (!kMono<FMT>) if (tx < g.W && ty < g.H) {
                const Tap4 tc = colT[tx], tr = rowT[ty];
                for (int a = 0; a < 4; ++a) {
                    if (tr.w[a] == 0.0f) continue;
                    const int sr = wrap_near(tr.idx[a], g.H, g.edge);
                    float hi = 0.0f, hq = 0.0f;
                    for (int b = 0; b < 4; ++b) {
                        const int sc = wrap_near(tc.idx[b], g.W, g.edge);
                        if constexpr (kRGB24<FMT>) {   // RGBA8's expression on the pixel's RGBA8 word
                            const float2 iq = chroma_iq<0>(
                                rgb24_canon(rgb24_px(img, (unsigned)sr * g.li.pitch, (unsigned)sc, g), g));
                            hi += tc.w[b] * iq.x;
                            hq += tc.w[b] * iq.y;
                        } else {
                            const float2 iq = chroma_iq<FMT>(ld_off<typename Pix<FMT>::raw_t>(
                                img, (unsigned)sr * g.li.pitch + (unsigned)sc * Pix<FMT>::bpp));
                            hi += tc.w[b] * iq.x;
                            hq += tc.w[b] * iq.y;
                        }
                    }
                    ci += tr.w[a] * hi;
                    cq += tr.w[a] * hq;
                }
            }
            acc[0] += wt * sat(1.0f * yb + 0.956f * ci + 0.621f * cq);
            acc[1] += wt * sat(1.0f * yb + -0.272f * ci + -0.647f * cq);
            acc[2] += wt * sat(1.0f * yb + -1.106f * ci + 1.703f * cq);
        }
    uint8_t *row = frames_out + (size_t)frame * g.lo.stride + (size_t)((unsigned)Y * g.lo.pitch);
    // gray: R = G = B = the mean of the texels' sat(Y'), whose luma is itself
    if constexpr (kMono<FMT>) mono_store<FMT>(row, (unsigned)X, acc[0], g);
    else if constexpr (kRGB24<FMT>) rgb24_store(row, (unsigned)X, acc[0], acc[1], acc[2], g);
    else Pix<FMT>::store(row, (unsigned)X, acc[0], acc[1], acc[2]);
}

// =========================================================================
// f3 debug views: ProcessDebugView (.cs:234-257)
// =========================================================================
// The reference shows complexBuffer1 after PerformFFT, which its ping-pong
// (.cs:517-549) leaves one radix-2 column stage short of the spectrum: with
// R[r][kx] = (-1)^r Frow[r][(kx + N/2) mod N] (centred, row-transformed), rows
// [0, N/2) hold the N/2-point column DFT of the even rows r = 2m and rows
// [N/2, N) that of the odd rows (oracle mm_ref_fft_buffer1, tests/np_twin.py).
// One WG per (frame, column kx): group 0 transforms the even rows, group 1 the
// odd rows (T/2 threads each, N/2-point FFT).  Frow comes from K1's half
// spectra G (Hermitian: Frow[r][f] = conj G[N-f][r] for f > N/2; rows outside
// the image are zero).  Chunk frame fr = frame0 + blockIdx / N reads G[fr] and
// writes view texture fr - frame0.  Writes the log-magnitude view
// (ConvertComplexMagToTexScaled, FFT.compute:152-161) and/or the phase view
// (ConvertComplexPhaseToTex, :164-172) as N x N float textures.
template <int LOG2N>
__global__ __launch_bounds__(2 * fft_T<LOG2N - 1>())
void k_dbg_cols(const c2 *__restrict__ G, size_t g_stride, float *__restrict__ tex,
                size_t tex_stride, int frame0, int want_mag, int want_phase, Geo g,
                const c2 *__restrict__ tw_half)
{
    constexpr int N = 1 << LOG2N, M = N / 2, T = fft_T<LOG2N - 1>();
    extern __shared__ __attribute__((aligned(16))) c2 lds_all[];
    const int grp = threadIdx.x / T, t = threadIdx.x % T;   // 0: even rows, 1: odd rows
    c2 *lds = lds_all + grp * lds_complex<M>();
    const int kx = blockIdx.x % N, fr = frame0 + blockIdx.x / N;
    const int f = (kx + N / 2) & (N - 1);
    const bool mirror = f > N / 2;
    const c2 *Gc = G + (size_t)fr * g_stride + (size_t)(mirror ? N - f : f) * g.Hg;
    const float sgn = grp ? -1.0f : 1.0f;                     // (-1)^r
    c2 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int r = 2 * (t + j * T) + grp;                   // canvas row
        const int rr = r - g.y0;
        const c2 a = Gc[min(max(rr, 0), g.H - 1)];
        const bool in = rr >= 0 && rr < g.H;
        v[j] = in ? mk(sgn * a.x, sgn * (mirror ? -a.y : a.y)) : mk(0.0f, 0.0f);
    }
    fft_regs<LOG2N - 1, -1>(v, t, lds, tw_half);
    float *mag = tex + (size_t)(fr - frame0) * tex_stride;
    float *pha = mag + (size_t)N * N;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int row = grp * M + t + j * T;
        const float m2 = v[j].x * v[j].x + v[j].y * v[j].y;
        if (want_mag) mag[(size_t)row * N + kx] = __log10f(__builtin_amdgcn_sqrtf(m2) * 10.0f + 1.0f) * 0.25f;
        if (want_phase) pha[(size_t)row * N + kx] = fabsf(atan2f(v[j].y, v[j].x)) * (1.0f / 1.57079632679f);
    }
}

// CropTexture (.cs:386-410) of one view, or ShowSplitScreen (.cs:458-487) of
// both (each N x N texture drawn bilinearly into one half).  RFloat textures
// sample as (v, 0, 0, 1).
template <int FMT>
__global__ __launch_bounds__(256)
void k_dbg_out(const float *__restrict__ tex, size_t tex_stride, uint8_t *__restrict__ frames_out,
               int frame0, int nframes, int show_mag, int show_phase, Geo g)
{
    const size_t npx = (size_t)g.W * g.H;
    const size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (e >= npx * nframes) return;
    const int k = (int)(e / npx);
    const int p = (int)(e - (size_t)k * npx);
    const int Y = p / g.W, X = p - Y * g.W;
    const float *mag = tex + (size_t)k * tex_stride, *pha = mag + (size_t)g.N * g.N;
    float v;
    if (show_mag && show_phase) {
        const bool right = 2 * X + 1 >= g.W;
        const float u = (float)(2 * X + 1 - (right ? g.W : 0)) / (float)g.W;
        const float vv = (float)(2 * Y + 1) / (float)(2 * g.H);
        const float *tx = right ? pha : mag;
        // bilinear at texel (u N - 0.5, v N - 0.5), sampler wrap = edge mode
        const float sx = u * (float)g.N - 0.5f, sy = vv * (float)g.N - 0.5f;
        const float fx0 = floorf(sx), fy0 = floorf(sy);
        const float ax = sx - fx0, ay = sy - fy0;
        const int ix = (int)fx0, iy = (int)fy0;
        const int xa = wrap_idx(ix, g.N, g.edge), xb = wrap_idx(ix + 1, g.N, g.edge);
        const int ya = wrap_idx(iy, g.N, g.edge), yb = wrap_idx(iy + 1, g.N, g.edge);
        const float a = (1.0f - ax) * tx[(size_t)ya * g.N + xa] + ax * tx[(size_t)ya * g.N + xb];
        const float b = (1.0f - ax) * tx[(size_t)yb * g.N + xa] + ax * tx[(size_t)yb * g.N + xb];
        v = (1.0f - ay) * a + ay * b;
    } else {
        v = (show_mag ? mag : pha)[(size_t)(g.y0 + Y) * g.N + g.x0 + X];
    }
    if (kUnorm<FMT> || kMono<FMT> || kRGB24<FMT>) v = sat(v);   // UNORM destination
    uint8_t *row = frames_out + (size_t)(frame0 + k) * g.lo.stride + (size_t)((unsigned)Y * g.lo.pitch);
    // a gray frame holds the R channel the view is: the code of its value
    if constexpr (kMono<FMT>) mono_store<FMT>(row, (unsigned)X, v, g);
    else if constexpr (kRGB24<FMT>) rgb24_store(row, (unsigned)X, v, 0.0f, 0.0f, g);   // (the RGBA8 view's R, G, B)
    else Pix<FMT>::store(row, (unsigned)X, v, 0.0f, 0.0f);
}

// =========================================================================
// passthrough of pitched frames (the first frame, apply_magnification = 0)
// =========================================================================
// One workgroup per (plane row, frame): the row's samples and nothing else, in
// words of U (NV12 and the 16-bit single-plane formats: 2 bytes, their unit;
// MM_Y8 and packed RGB: 1; every other format: 4, which divides its unit; packed 4:2:2: 4, one macropixel or, MM_Y210, half of one).  `rows_y` RGBA / luma rows, then the (Cb, Cr) rows of a 4:2:0
// frame.  Tight frames on both sides are one plain device copy instead.
template <class U>
__global__ __launch_bounds__(256)
void k_copy_rows(const uint8_t *__restrict__ frames_in, uint8_t *__restrict__ frames_out, Geo g,
                 unsigned row_bytes, int rows_y)
{
    const int r = blockIdx.x, c = r - rows_y;
    const uint8_t *src = frames_in + (size_t)blockIdx.y * g.li.stride +
                         (c < 0 ? (size_t)((unsigned)r * g.li.pitch) : (size_t)(g.li.c_off + (unsigned)c * g.li.c_pitch));
    uint8_t *dst = frames_out + (size_t)blockIdx.y * g.lo.stride +
                   (c < 0 ? (size_t)((unsigned)r * g.lo.pitch) : (size_t)(g.lo.c_off + (unsigned)c * g.lo.c_pitch));
    for (unsigned o = threadIdx.x * (unsigned)sizeof(U); o < row_bytes; o += 256u * (unsigned)sizeof(U))
        st_off<U>(dst, o, ld_off<U>(src, o));
}

// =========================================================================
// plain conversion between two formats (mm_process_convert's passthrough frames)
// =========================================================================
// Where the formats of the two sides differ, the frames that pass through (the
// first frame, apply_magnification = 0, the seed frame of a stream) cannot be
// copied: they are converted, the out rule applied to the saturated RGBA32F
// frame the in frame IS (include/mm.h).  One launch for n frames, one lane per
// block of 4 x 2 pixels, so that the two (Cb, Cr) pairs of a 4:2:0 side stay
// in the lane: FMT is one of the three mixed pairs.
//   NV12 in:  two luma dwords and one chroma dword, two 16-byte stores
//   P010 in:  two 8-byte luma loads and two 4-byte chroma loads (c420_quad_pairs)
//   RGBA8 in: two 16-byte loads, two luma dwords and one chroma dword out
// QUAD: W % 4 == 0 and every row of every frame of the launch on a multiple of
// 4 bytes on the 8-bit 4:2:0 side (convert_quads_aligned, mm_impl.hpp); the
// multi-dword accesses are typed with the alignment they have (ld_quad_a4).
// !QUAD: the same lane, the same arithmetic, single samples, pairs and pixels,
// and the columns of the block that lie inside W (W is even: two or four).
// The decode is the format's matrix in fp32, not the YIQ detour: the decode's
// coefficients over the chroma code scale come in Cvt (Geo has no field for
// them), the luma scale and every output weight in Geo::nv.  Nothing outside
// the W x H samples is read or written.
struct Cvt {
    float rcr, gcb, gcr, bcb;   // R = y + rcr (Cr - mid), G = y + gcb (Cb - mid) + gcr (Cr - mid), B = y + bcb (Cb - mid)
};
template <int FMT, bool QUAD>
__global__ __launch_bounds__(256)
void k_convert(const uint8_t *__restrict__ frames_in, uint8_t *__restrict__ frames_out, Geo g, Cvt cv, int nframes)
{
    constexpr int FI = kFmtIn<FMT>, FO = kFmtOut<FMT>;
    static_assert(FMT >= 256 && kFmtPairOk<FMT>, "one of the mixed pairs");
    const unsigned bw = (unsigned)(g.W + 3) / 4u;            // blocks per row pair
    const size_t nb = (size_t)bw * (unsigned)(g.H / 2);     // ... per frame
    const size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (e >= nb * (size_t)nframes) return;
    const unsigned frame = (unsigned)(e / nb), p = (unsigned)(e - (size_t)frame * nb);
    const unsigned by = p / bw, X = (p - by * bw) * 4u, Y = by * 2u;
    const int nc = QUAD ? 4 : min(4, g.W - (int)X);          // columns of the block inside W: 4 or 2
    const uint8_t *img = frames_in + (size_t)frame * g.li.stride;
    uint8_t *outp = frames_out + (size_t)frame * g.lo.stride;

    float rr[2][4], gg[2][4], bb[2][4];   // the block's saturated RGB
    if constexpr (k420<FI>) {
        constexpr unsigned sb = kP010<FI> ? 2u : 1u;           // bytes per sample
        constexpr float mid = kP010<FI> ? 32768.0f : 128.0f;   // neutral chroma, in the sample's units
        float yv[2][4];
        unsigned pr[2];   // the block's two (Cb, Cr) pairs
        [[maybe_unused]] const unsigned coff = g.li.c_off + by * g.li.c_pitch + X * sb;
        if constexpr (QUAD) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const unsigned off = (Y + r) * g.li.pitch + X * sb;
                if constexpr (kP010<FI>) {
                    const uint2 w = ld_pair_a4(img, off);
                    yv[r][0] = (float)(w.x & 0xFFFFu); yv[r][1] = (float)(w.x >> 16);
                    yv[r][2] = (float)(w.y & 0xFFFFu); yv[r][3] = (float)(w.y >> 16);
                } else {
                    const unsigned w = ld_off<uint32_t>(img, off);
#pragma unroll
                    for (int k = 0; k < 4; ++k) yv[r][k] = (float)((w >> (8 * k)) & 255u);
                }
            }
            c420_quad_pairs<FI>(img, g, (int)Y, X, pr[0], pr[1]);
        } else {
            using luma_t = typename LumaSrc<FI>::raw_t;
            using pair_t = typename ChromaSrc<FI>::raw_t;
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    yv[r][k] = k < nc ? (float)ld_off<luma_t>(img, (Y + r) * g.li.pitch + (X + k) * sb) : 0.0f;
            pr[0] = ld_off<pair_t>(img, coff);
            pr[1] = nc > 2 ? (unsigned)ld_off<pair_t>(img, coff + 2u * sb) : pr[0];
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float cb, cr;
            if constexpr (kP010<FI>) cb = (float)(pr[j] & 0xFFFFu) - mid, cr = (float)(pr[j] >> 16) - mid;
            else cb = (float)(pr[j] & 255u) - mid, cr = (float)((pr[j] >> 8) & 255u) - mid;
            const float dr = cv.rcr * cr, dg = cv.gcb * cb + cv.gcr * cr, db = cv.bcb * cb;
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int k = 2 * j; k < 2 * j + 2; ++k) {
                    const float y = (yv[r][k] - g.nv.y_off) * g.nv.y_unit;
                    rr[r][k] = sat(y + dr); gg[r][k] = sat(y + dg); bb[r][k] = sat(y + db);
                }
        }
    } else {   // RGBA8 / BGRA8 in: byte / 255 (in [0, 1] already), alpha ignored
        static_assert(kRGBA8u<FI>, "the 4-byte side of a mixed pair is MM_RGBA8 or MM_BGRA8");
        constexpr float s = 1.0f / 255.0f;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const unsigned off = (Y + r) * g.li.pitch + X * 4u;
            unsigned px[4];
            if constexpr (QUAD) {
                const uint4 m = ld_quad_a4(img, off);
                px[0] = m.x; px[1] = m.y; px[2] = m.z; px[3] = m.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) px[k] = k < nc ? ld_off<uint32_t>(img, off + 4u * k) : 0u;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                rr[r][k] = (float)((px[k] >> Pix<FI>::rs) & 255u) * s;
                gg[r][k] = (float)((px[k] >> 8) & 255u) * s;
                bb[r][k] = (float)((px[k] >> Pix<FI>::bs) & 255u) * s;
            }
        }
    }

    if constexpr (kRGBA8u<FO>) {   // RGBA8 / BGRA8 out: Pix<FO>::pack, alpha 255
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            uint8_t *row = outp + (size_t)((Y + r) * g.lo.pitch);
            if constexpr (QUAD) {
                uint4 px;
                px.x = Pix<FO>::pack(rr[r][0], gg[r][0], bb[r][0]);
                px.y = Pix<FO>::pack(rr[r][1], gg[r][1], bb[r][1]);
                px.z = Pix<FO>::pack(rr[r][2], gg[r][2], bb[r][2]);
                px.w = Pix<FO>::pack(rr[r][3], gg[r][3], bb[r][3]);
                st_stream_quad_a4(row, X * 4u, px);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < nc) st_off<uint32_t>(row, (X + k) * 4u, Pix<FO>::pack(rr[r][k], gg[r][k], bb[r][k]));
            }
        }
    } else {   // NV12 out: the compose kernels' codes (nv12_ycode, nv12_ccode) and their order of sums
        static_assert(kNV12<FO>, "the 4:2:0 destination of a mixed pair is NV12");
        c2 cd[2][4];
        unsigned yc[2][4];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k = 0; k < 4; ++k) yc[r][k] = nv12_ycode(rr[r][k], gg[r][k], bb[r][k], g, cd[r][k]);
        const c2 b0 = (cd[0][0] + cd[1][0]) + (cd[0][1] + cd[1][1]), b1 = (cd[0][2] + cd[1][2]) + (cd[0][3] + cd[1][3]);
        const unsigned c0 = nv12_ccode(b0.x, g.nv.cbo) | nv12_ccode(b0.y, g.nv.cro) << 8;
        const unsigned c1 = nv12_ccode(b1.x, g.nv.cbo) | nv12_ccode(b1.y, g.nv.cro) << 8;
        uint8_t *crow = outp + (size_t)(g.lo.c_off + by * g.lo.c_pitch);
        if constexpr (QUAD) {
#pragma unroll
            for (int r = 0; r < 2; ++r)
                st_stream<uint32_t>(outp + (size_t)((Y + r) * g.lo.pitch), X,
                                    yc[r][0] | yc[r][1] << 8 | yc[r][2] << 16 | yc[r][3] << 24);
            st_stream<uint32_t>(crow, X, c0 | c1 << 16);
        } else {
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < nc) st_off<uint8_t>(outp + (size_t)((Y + r) * g.lo.pitch), X + k, (uint8_t)yc[r][k]);
            st_off<uint16_t>(crow, X, (uint16_t)c0);
            if (nc > 2) st_off<uint16_t>(crow, X + 2u, (uint16_t)c1);
        }
    }
}

// =========================================================================
// synthetic stream, RGBA8
// =========================================================================
__device__ __forceinline__ uint64_t splitmix64(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static __global__ void k_synth(uint8_t *out, int W, int H, int t0, int count, uint64_t seed, int gray)
{
    const size_t npx = (size_t)W * H;
    const size_t total = npx * count;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total;
         e += (size_t)gridDim.x * blockDim.x) {
        const int fr = (int)(e / npx);
        const size_t p = e - (size_t)fr * npx;
        const int y = (int)(p / W), x = (int)(p - (size_t)y * W);
        const double two_pi = 6.283185307179586;
        const double d = 0.5 * sin(two_pi * 0.05 * (t0 + fr));
        const double sx = sin(two_pi * (x + d) / 37.0), cy = cos(two_pi * y / 53.0);
        const double gc[3] = {1.0, 0.8, 0.6};
        uint32_t packed = 255u << 24;
        for (int ch = 0; ch < 3; ++ch) {
            const int cc = gray ? 0 : ch;
            const uint64_t h = splitmix64(seed ^ ((uint64_t)p * 3u + (uint64_t)cc));
            const double u = (double)(h >> 40) * (1.0 / 16777216.0);
            double v = 0.4 + 0.3 * sx * cy * gc[cc] + 0.15 * u;
            v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
            packed |= (uint32_t)floor(v * 255.0 + 0.5) << (8 * ch);
        }
        reinterpret_cast<uint32_t *>(out)[e] = packed;
    }
}

}  // namespace mm
