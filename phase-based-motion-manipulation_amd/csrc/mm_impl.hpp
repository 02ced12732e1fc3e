// mm_impl.hpp — the handle and the per-padded-size host drivers of the C-ABI
// (include/mm.h), shared by the translation units: mm_api.hip (the entry
// points and the size dispatch) and mm_n<L>.hip (one per log2 of the padded
// size N: the kernels of that size are instantiated there, so that a build
// compiles the sizes in parallel).
#pragma once
#if (defined(MM_K2_STAMPS) || defined(MM_K34_STAMPS)) && !defined(MM_ONLY_LOG2N)
#error "stamp builds are one-size builds: compile csrc/mm_api.hip alone with -DMM_ONLY_LOG2N=<log2 N>"
#endif
// C-ABI implementation (include/mm.h) of the MI355X-native
// MotionMagnificationProcessor frame operator.
//
// Reference surface (Assets/Scripts/MotionMagnificationProcessor.cs):
//   Start/InitializeProcessor :90-94,:289-342 -> mm_create
//   OnValidate                :78-88          -> mm_set_params
//   OnRenderImage             :101-143        -> mm_process / mm_process_stream
//   OnDestroy/ReleaseResources:96-99,:344-356 -> mm_destroy
// There is no CPU fallback: every frame is computed by the HIP kernels of
// mm_kernels.hpp; without a gfx950 device mm_create fails with MM_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/mm.h"
#include "mm_steer.hpp"

using namespace mm;

#define HIPCHK(x)                                                             \
    do {                                                                      \
        hipError_t e_ = (x);                                                  \
        if (e_ != hipSuccess) {                                               \
            if (getenv("MM_DEBUG"))                                           \
                fprintf(stderr, "mm355: %s failed: %s (%s:%d)\n", #x,         \
                        hipGetErrorString(e_), __FILE__, __LINE__);           \
            return MM_ERR_HIP;                                                \
        }                                                                     \
    } while (0)

struct mm_handle {
    int W, H, N, log2n, device;
    mm_params p;
    hipStream_t stream;
    Geo geo;
    Spec spec;
    Blur5 blur;
    Tap4 *d_col, *d_row;
    float4 *d_col3, *d_row3;    // the same taps merged onto offsets -1, 0, +1
    c2 *d_tw;
    float2 *d_ktab;             // K2's per-bin tables of every column (k_k2_table)
    float *d_kmsum;             // ... and the bins' whole mask sums (pyramid tables)
    int ktab_mode;              // table kind d_ktab holds (-1: stale, refilled before the next K2)
    c2 *d_tw_half;              // W_{N/2} table (debug views, lazily)
    float *d_dbg;               // debug view textures [dbg_frames][mag, phase][N][N] (lazily)
    // MM_MODE_STEERABLE (lazily, for the current levels/orientations):
    c2 *d_Fb;                   // per batch frame half spectrum [fb_frames][N/2+1][N] (lazily)
    c2 *d_T;                    // band rows [nb+1][t_rows(Hn)][N] (row groups, MM_SB_RROWS; k_sb_cols -> k_sb_rows)
    float *d_sst;               // temporal-filter state: phi, u_h, u_l planes [nb][Hn][W+4]
    int steer_nb;               // bands the steerable buffers were sized for (-1: none)
    int steer_planes;           // state planes allocated (1: DIFF, 3: IIR)
    int sb_nf;                  // frames per k_sb_rows launch (MM_SB_NF; 2: pairs)
    int sb_cf;                  // frames per k_sb_cols launch at N <= 2048 (MM_SB_CF)
    bool steer_valid;           // d_sst holds the state after the previous frame
    // G: chunk + 1 slots of K1's row spectra.  Slot gs holds G_{t-1}, the row
    // spectra of the previous input frame: the temporal state
    // (previousSourceTexture, .cs:142), valid while has_state.  A batch's
    // frames go to slots that avoid gs (place_batch).
    c2 *d_G, *d_Q;
    float *d_Yh;                // unfused K3 -> K4 / steerable rows (lazily, yh_frames)
    size_t g_stride, q_stride, yh_stride;  // elements per frame
    int chunk;                  // frames per K1/K2/K3 batch (mm_set_batch)
    int gs;                     // G slot of the state
    int yh_frames, fb_frames, dbg_frames;  // frames the lazy buffers hold
    hipEvent_t last_ev;         // recorded after this handle's latest work (mm_set_params)
    hipEvent_t retire_ev;       // orders a buffer's return to the pool behind a call's stream
    bool last_ev_set;
    hipStream_t last_s;         // the stream last_ev was recorded on
    bool k2_tab;                // pyramid masks from the per-bin LDS table (<= 2 bands/bin)
    bool k2_tab2;               // ... with overlapping middle bands (MM_K2_PYR_TAB2)
    uint8_t *d_stage_in, *d_stage_out;
    size_t stage_bytes;
    bool has_state;
    bool hold;                  // frames pair with the state and do not advance it (mm_set_hold)
    bool g_valid;               // the G slot gs holds G_{t-1} (K1 or a non-steerable mm_set_state
                                // wrote it; a steerable mm_set_state sets only the local phases)
    int k2_tail_pct;            // share of a batch's frames of k_cols's packed block run by k_cols_tail
    int k2_tail2_pct;           // share of the second-half blocks' frames run by k_cols's tail blocks
    int k34_rows;               // output rows per k_rows_inv_compose strip (0: K3 + K4 unfused;
                                // -1: by the launch's frame count, k34_strip_rows)
    int k34_oneshot;            // short launches: k_rows_inv_compose4 when its strips fit one
                                // workgroup round (MM_K34_ONESHOT: 0 never: K3 -> K4, 2 always)
    int num_cu;                 // compute units of the device
    // Lanes (mm_set_lanes): the temporal states of `lanes` live streams, apart
    // from the handle's own state above; a call (mm_process_lanes_mask)
    // advances the lanes of its mask by one frame each.  d_LG: two banks of
    // `lanes` G slots.  Bit k of lane_bank: the bank whose slot k holds lane
    // k's G_{t-1}.  A call's K1 writes a selected lane's other slot, its K2
    // reads both, then that lane's bit flips: no state copy, and a lane that
    // sits a call out keeps its slot.  d_LQ: a Q slot per lane.  Bit k of
    // lane_state: lane k has state.  d_Lsrc (lazily, lsrc_bytes): the source
    // frames of a lane call whose in and out overlap, tight, for its compose.
    int lanes;
    c2 *d_LG, *d_LQ;
    uint64_t lane_bank;
    uint64_t lane_state;
    uint64_t lane_hold;         // bit k: lane k holds its reference (mm_set_lanes_hold)
    uint8_t *d_Lsrc;
    size_t lsrc_bytes;
    // mm_profile_begin/end: HIP events around each launch on its stream
    struct ProfRec { hipEvent_t a, b; int kernel, frames; };
    bool prof;
    std::vector<ProfRec> prof_recs;
};

// Makes the handle's device current for the scope of an entry point and gives
// the caller's current device back on the way out (a multi-GPU host or an
// engine plugin keeps its own device selection across mm_* calls).
struct DeviceScope {
    int prev = -1;
    hipError_t err;
    explicit DeviceScope(int dev)
    {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) err = hipSetDevice(dev);
        else if (err == hipSuccess) prev = -1;   // already current: nothing to restore
    }
    ~DeviceScope()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};
#define DEVICE_SCOPE(h)                                  \
    DeviceScope dev_scope_((h)->device);                 \
    if (dev_scope_.err != hipSuccess) return MM_ERR_HIP

// Device memory of a handle comes from the device's stream-ordered pool
// (hipMallocAsync on the handle's own stream) and goes back with hipFreeAsync
// ordered behind the handle's own work: hipFree would synchronise the whole
// device (hip_runtime_api.h: "implicit hipDeviceSynchronize"), stalling every
// other handle and stream on the GPU at a teardown or a batch change
// (VERDICT r3 #6).  An allocation is made usable on every stream by waiting
// for the handle's stream (nothing else is queued there).
// A failed allocation leaves no error behind: the next launch check
// (hipGetLastError) would otherwise report it as that launch's failure (an
// OOM from mm_set_batch must leave the handle usable).
template <class T>
static hipError_t h_alloc(mm_handle *h, T **p, size_t bytes)
{
    hipError_t e = hipMallocAsync(reinterpret_cast<void **>(p), bytes, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        if (*p && e != hipErrorOutOfMemory) (void)hipFreeAsync(*p, h->stream);
        *p = nullptr;
        (void)hipGetLastError();
    }
    return e;
}

// Returns a buffer to the pool once this handle's work that may read it is
// done: the handle's last call (last_ev) and, when given, what the current
// call has queued on its stream s so far.  No host wait.
static void h_retire(mm_handle *h, void *p, hipStream_t s = nullptr, bool have_s = false)
{
    if (!p) return;
    if (h->last_ev_set) (void)hipStreamWaitEvent(h->stream, h->last_ev, 0);
    if (have_s && s != h->stream && hipEventRecord(h->retire_ev, s) == hipSuccess)
        (void)hipStreamWaitEvent(h->stream, h->retire_ev, 0);
    (void)hipFreeAsync(p, h->stream);
}

// Marks the end of this handle's latest work on stream s (mm_set_params waits
// for it before rewriting the tables that work may read).
static int note_work(mm_handle *h, hipStream_t s)
{
    HIPCHK(hipEventRecord(h->last_ev, s));
    h->last_ev_set = true;
    h->last_s = s;
    return MM_OK;
}

// A call on another stream than the handle's previous call first waits for
// that call's work (last_ev), so last_ev always covers every earlier call and
// the buffers h_retire returns behind it are not still read on the old stream.
// Same stream (the one-frame drop-in pattern): nothing to do.
static int order_after_last(mm_handle *h, hipStream_t s)
{
    if (h->last_ev_set && s != h->last_s) HIPCHK(hipStreamWaitEvent(s, h->last_ev, 0));
    return MM_OK;
}

// Brackets one kernel launch with events when profiling is on.
struct ProfScope {
    mm_handle *h;
    hipStream_t s;
    mm_handle::ProfRec r;
    bool on;
    ProfScope(mm_handle *h_, hipStream_t s_, int kernel, int frames) : h(h_), s(s_), on(h_->prof)
    {
        if (!on) return;
        r.kernel = kernel;
        r.frames = frames;
        // timing only: a device-scope release (no system-scope cache write-back
        // between the kernels being timed)
        on = hipEventCreateWithFlags(&r.a, hipEventDisableSystemFence) == hipSuccess &&
             hipEventCreateWithFlags(&r.b, hipEventDisableSystemFence) == hipSuccess &&
             hipEventRecord(r.a, s) == hipSuccess;
    }
    ~ProfScope()
    {
        if (on && hipEventRecord(r.b, s) == hipSuccess) h->prof_recs.push_back(r);
    }
};

// The formats: one row each in mm_format.hpp (fmt_info; null: no format).  A
// 4:2:0 or packed 4:2:2 code may carry one matrix bit (MM_MATRIX_BT709 /
// MM_MATRIX_BT2020): layout, sizes and units are its row's, the bit changes
// coefficients (geo_of) and K1's instance (MM_FMT_SWITCH_K1).
#include "mm_format.hpp"
// What every frame entry point asks of (format, geometry, parameters) before
// it queues anything.  The Y'CbCr formats are subsampled: even sizes only
// (4:2:2: even H too, include/mm.h); the debug views are R-channel pictures,
// which they cannot hold.  (The single-plane formats hold them, and have no
// subsampling: every size, every view.)
static inline int fmt_check(int W, int H, int fmt, const mm_params *p)
{
    const FmtInfo *f = fmt_info(fmt);
    if (!f) return MM_ERR_INVALID;
    if (f->ycc() && ((W | H) & 1)) return MM_ERR_UNSUPPORTED;
    if (f->ycc() && p && (p->show_magnitude || p->show_phase)) return MM_ERR_UNSUPPORTED;
    return MM_OK;
}
// ---- surfaces (mm_surface, include/mm.h) ----------------------------------
// Three-plane 4:2:0: the Cr plane's offset from the Cb plane (include/mm.h:
// derived, mm_surface has one chroma offset)
static inline size_t i420_cr_delta(int H, size_t chroma_pitch) { return chroma_pitch * (size_t)(H / 2); }
static inline int surf_tight(int W, int H, int fmt, mm_surface *s)
{
    if (!s || W < 1 || H < 1) return MM_ERR_INVALID;
    if (int rc = fmt_check(W, H, fmt, nullptr)) return rc;
    const FmtInfo &f = *fmt_info(fmt);
    s->format = fmt;
    s->pitch = f.tight_pitch(W);   // (the row's bytes; v210: rounded up to 128)
    s->chroma_offset = f.planes > 1 ? s->pitch * (size_t)H : 0;
    s->chroma_pitch = f.planes > 1 ? f.chroma_row_bytes(W) : 0;
    s->frame_stride = f.frame_bytes(W, H);
    return MM_OK;
}
// The largest extent the kernels' 32-bit byte offsets from a frame's base
// reach (ld_off / st_off / st_stream take `unsigned`): every sample below 2^32.
static constexpr unsigned long long kSurfMaxExtent = 1ull << 32;
// mm_surface_bytes: the layout's validation and its extent (host only)
static inline int surf_check(int W, int H, const mm_surface *s, size_t *extent)
{
    if (!s || W < 1 || H < 1) return MM_ERR_INVALID;
    if (int rc = fmt_check(W, H, s->format, nullptr)) return rc;
    const size_t u = fmt_info(s->format)->unit;
    Plane pl[3];
    const int np = surf_planes(W, H, *s, pl);
    if (!np || (np == 1 && (s->chroma_offset || s->chroma_pitch))) return MM_ERR_INVALID;
    size_t end = 0;   // the byte after the last sample of the planes so far
    for (int k = 0; k < np; ++k) {
        const Plane &q = pl[k];
        if (q.pitch < q.row_bytes || q.pitch % u || q.offset % u || q.offset < end) return MM_ERR_INVALID;
        if (__builtin_mul_overflow(q.pitch, q.rows - 1, &end) || __builtin_add_overflow(end, q.offset, &end) ||
            __builtin_add_overflow(end, q.row_bytes, &end))
            return MM_ERR_INVALID;
    }
    if (end > kSurfMaxExtent) return MM_ERR_UNSUPPORTED;
    if (extent) *extent = end;
    return MM_OK;
}
// What a frame entry point asks of `count` frames at `p` in layout `s`
// (host-memory frames go through copies into aligned staging buffers: their
// pointers need no alignment, as before)
static inline int surf_check_frames(int W, int H, const void *p, const mm_surface *s, int count,
                                    bool on_device = true)
{
    size_t extent;
    if (int rc = surf_check(W, H, s, &extent)) return rc;
    const size_t u = fmt_info(s->format)->unit;
    if (on_device && reinterpret_cast<uintptr_t>(p) % u) return MM_ERR_INVALID;
    if (count > 1 && (s->frame_stride < extent || s->frame_stride % u)) return MM_ERR_INVALID;
    return MM_OK;
}
static inline Geo::Lay surf_lay(const mm_surface &s)
{
    Geo::Lay l;
    l.pitch = (unsigned)s.pitch;            // (< 2^32 wherever a second row exists: extent <= 2^32)
    l.c_off = (unsigned)s.chroma_offset;
    l.c_pitch = (unsigned)s.chroma_pitch;
    l.yb = 0;
    l.stride = s.frame_stride;
    return l;
}
// The pairs of different formats mm_process_convert takes (include/mm.h):
// decode, any NV12 or P010 code to MM_RGBA8; encode, MM_RGBA8 to any NV12 code;
// and both with MM_BGRA8 as the 4-byte side.
static inline int convert_supported(int in_fmt, int out_fmt)
{
    const FmtInfo *fi = fmt_info(in_fmt), *fo = fmt_info(out_fmt);
    if (!fi || !fo) return MM_ERR_INVALID;
    if (in_fmt == out_fmt) return MM_OK;
    // (a three-plane code has no mixed pair)
    if ((fi->kfmt == kFmtNV12 || fi->kfmt == kFmtP010) && (out_fmt == MM_RGBA8 || out_fmt == MM_BGRA8)) return MM_OK;
    if ((in_fmt == MM_RGBA8 || in_fmt == MM_BGRA8) && fo->kfmt == kFmtNV12) return MM_OK;
    return MM_ERR_UNSUPPORTED;
}
// The frames of one call: their formats and where the two sides lie.  fmt is
// the input side's (K1, the state and every same-format path read it alone),
// ofmt the output side's: the same but in a convert call.
struct Frames {
    int fmt, ofmt;
    const FmtInfo *fi, *fo;   // their rows, looked up once per call
    Geo::Lay in, out;
    size_t fb;       // mm_frame_bytes (of fmt)
    bool packed;     // one format, both sides tight, frames back to back: a passthrough is one plain copy
    bool mixed() const { return fmt != ofmt; }
};
static inline Frames frames_of(int W, int H, const mm_surface &li, const mm_surface &lo)
{
    Frames f;
    f.fmt = li.format;
    f.ofmt = lo.format;
    f.fi = fmt_info(f.fmt);
    f.fo = fmt_info(f.ofmt);
    f.in = surf_lay(li);
    f.out = surf_lay(lo);
    f.fb = f.fi->frame_bytes(W, H);
    mm_surface t;
    (void)surf_tight(W, H, f.fmt, &t);
    auto tight = [&](const mm_surface &s) {
        return s.pitch == t.pitch && s.chroma_offset == t.chroma_offset && s.chroma_pitch == t.chroma_pitch &&
               s.frame_stride == t.frame_stride;
    };
    // (a tight v210 frame whose rows end before its pitch has padding of its
    // own, which a plain copy would carry along: k_copy_rows)
    f.packed = !f.mixed() && tight(li) && tight(lo) && t.pitch == f.fi->row_bytes(W);
    return f;
}

// One case of a format switch: the statement with the compile-time instance FMT_
#define MM_FMT_CASE(F, ...) case F: { constexpr int FMT_ = F; __VA_ARGS__; } break;
// Runs the statement with the compile-time format FMT_ of the row `fi`: its
// kernel instance (both ranges and every matrix of a Y'CbCr format run the one
// instance, the three word depths of the single-plane formats the MM_Y16
// instances, both byte orders of packed 4:2:2 the MM_YUY2 instances, both of
// packed RGB the MM_RGB24 instances; geo_of sets their uniforms).
#define MM_FMT_SWITCH(fi, ...)                                                 \
    switch ((fi)->kfmt) {                                                      \
    MM_FMT_CASE(MM_RGBA8, __VA_ARGS__)                                         \
    MM_FMT_CASE(MM_RGBA32F, __VA_ARGS__)                                       \
    MM_FMT_CASE(MM_RGBA16F, __VA_ARGS__)                                       \
    MM_FMT_CASE(kFmtNV12, __VA_ARGS__)                                         \
    MM_FMT_CASE(kFmtP010, __VA_ARGS__)                                         \
    MM_FMT_CASE(kFmtY8, __VA_ARGS__)                                           \
    MM_FMT_CASE(kFmtY16, __VA_ARGS__)                                          \
    MM_FMT_CASE(kFmtYUY2, __VA_ARGS__)                                         \
    MM_FMT_CASE(kFmtY210, __VA_ARGS__)                                         \
    MM_FMT_CASE(kFmtRGB24, __VA_ARGS__)                                        \
    MM_FMT_CASE(kFmtI420, __VA_ARGS__)                                         \
    MM_FMT_CASE(kFmtI010, __VA_ARGS__)                                         \
    MM_FMT_CASE(kFmtBGRA8, __VA_ARGS__)                                        \
    MM_FMT_CASE(kFmtBGRA8S, __VA_ARGS__)                                       \
    /* a grouped format has no instance of the kernels launched through this  \
       switch (its K1 and K4 launches name theirs): refused, never another    \
       format's kernel over its bytes */                                       \
    case kFmtV210: return MM_ERR_UNSUPPORTED;                                  \
    default: { constexpr int FMT_ = MM_RGBA8_SRGB; __VA_ARGS__; } break;       \
    }
// ... the compose kernels' (k_compose, k_rows_inv_compose, k_rows_inv_compose4):
// FMT_ is the pair's code for the frames of a convert call (mm_kernels.hpp
// fmt_pair; convert_supported leaves these six), else the format's
#define MM_MIXED_SWITCH(fr, ...)                                               \
    switch ((fr).fi->kfmt | ((fr).fo->kfmt == kFmtBGRA8 ? 256 : 0)) {          \
    case kFmtNV12: { constexpr int FMT_ = kFmtNV12toRGBA8; __VA_ARGS__; } break; \
    case kFmtP010: { constexpr int FMT_ = kFmtP010toRGBA8; __VA_ARGS__; } break; \
    case kFmtNV12 | 256: { constexpr int FMT_ = kFmtNV12toBGRA8; __VA_ARGS__; } break; \
    case kFmtP010 | 256: { constexpr int FMT_ = kFmtP010toBGRA8; __VA_ARGS__; } break; \
    case kFmtBGRA8: { constexpr int FMT_ = kFmtBGRA8toNV12; __VA_ARGS__; } break; \
    default: { constexpr int FMT_ = kFmtRGBA8toNV12; __VA_ARGS__; } break;     \
    }
#define MM_PAIR_SWITCH(fr, ...)                                                \
    do {                                                                       \
        if (!(fr).mixed()) { MM_FMT_SWITCH((fr).fi, __VA_ARGS__) }             \
        else { MM_MIXED_SWITCH(fr, __VA_ARGS__) }                              \
    } while (0);
// ... K1's: a code with a matrix bit runs its row's matrixed instance, which
// reads the chroma samples too (BT.709 and BT.2020, both ranges, share it): the
// chroma plane or planes, or whole macropixels (four bytes, or the 10-bit
// form's eight)
// (a grouped format, v210, has K1 instances and no fused compose instance, so
// MM_FMT_SWITCH refuses it: its row's two K1 instances are cases here, its
// compose launch_k4's)
#define MM_FMT_SWITCH_K1(fi, fmt, ...)                                         \
    switch (fmt_matrix(fmt) ? (fi)->k1m : (fi)->grp_px ? (fi)->kfmt : 0) {        \
    MM_FMT_CASE(kFmtV210, __VA_ARGS__)                                         \
    MM_FMT_CASE(kFmtV210M, __VA_ARGS__)                                        \
    MM_FMT_CASE(kFmtNV12M, __VA_ARGS__)                                        \
    MM_FMT_CASE(kFmtP010M, __VA_ARGS__)                                        \
    MM_FMT_CASE(kFmtI420M, __VA_ARGS__)                                        \
    MM_FMT_CASE(kFmtI010M, __VA_ARGS__)                                        \
    MM_FMT_CASE(kFmtYUY2M, __VA_ARGS__)                                        \
    MM_FMT_CASE(kFmtY210M, __VA_ARGS__)                                        \
    default: MM_FMT_SWITCH(fi, __VA_ARGS__)                                    \
    }
// K1's instance of a format: a single-plane frame IS a luma plane and runs the
// NV12 (bytes) or P010 (words) luma-plane instance with its own uniforms
// (geo_of: y_off 0, y_unit 1 / max), bit for bit what an instance of its own
// would compute (mm_kernels.hpp)
// (a BT.601 three-plane frame too: its luma plane is NV12's, so is the state;
// its 10-bit form's is P010's in another word unit, which the uniforms carry)
template <int F> constexpr int kK1Fmt = F == MM_Y8 || F == kFmtI420 ? kFmtNV12 : F == MM_Y16 || F == kFmtI010 ? kFmtP010 : F;
// ... and the kernels of the odd sizes and the debug views, which the Y'CbCr
// formats cannot have (refused by fmt_check before any launch): the RGBA, the
// packed RGB and the single-plane instances
#define MM_FMT_SWITCH_FULLRES(fi, ...)                                         \
    switch ((fi)->kfmt) {                                                      \
    MM_FMT_CASE(kFmtY8, __VA_ARGS__)                                           \
    MM_FMT_CASE(kFmtY16, __VA_ARGS__)                                          \
    MM_FMT_CASE(MM_RGBA8, __VA_ARGS__)                                         \
    MM_FMT_CASE(MM_RGBA32F, __VA_ARGS__)                                       \
    MM_FMT_CASE(MM_RGBA16F, __VA_ARGS__)                                       \
    MM_FMT_CASE(MM_RGBA8_SRGB, __VA_ARGS__)                                    \
    MM_FMT_CASE(kFmtRGB24, __VA_ARGS__)                                        \
    MM_FMT_CASE(kFmtBGRA8, __VA_ARGS__)                                        \
    MM_FMT_CASE(kFmtBGRA8S, __VA_ARGS__)                                       \
    default: return MM_ERR_UNSUPPORTED;                                        \
    }

// (Cb, Cr) -> (I, Q): RGBToYIQ's I and Q rows (RGBToYIQ.shader:46-50) times the
// BT.601 conversion R = y + 1.402 cr, G = y - 0.344136 cb - 0.714136 cr,
// B = y + 1.772 cb, in double: m = {I_cb, Q_cb, I_cr, Q_cr}.  (The y column
// of the product is the rows' sums, 0 for I and Q.)
// (Kr, Kb) of a matrix bit (include/mm.h)
static inline void matrix_krkb(int fmt, double *kr, double *kb)
{
    const int mx = fmt_matrix(fmt);
    *kr = mx == MM_MATRIX_BT709 ? 0.2126 : mx == MM_MATRIX_BT2020 ? 0.2627 : 0.299;
    *kb = mx == MM_MATRIX_BT709 ? 0.0722 : mx == MM_MATRIX_BT2020 ? 0.0593 : 0.114;
}
static inline void nv12_chroma_matrix(double m[4]);
// mm_ycbcr_matrix: (cb, cr) -> (Y, I, Q), m = {Y_cb, I_cb, Q_cb, Y_cr, I_cr,
// Q_cr}: RGBToYIQ's three rows (RGBToYIQ.shader:46-50) times the decode of the
// format's matrix, R = y + 2 (1 - Kr) cr, B = y + 2 (1 - Kb) cb, G = y -
// (2 Kb (1 - Kb) / Kg) cb - (2 Kr (1 - Kr) / Kg) cr, in double.  BT.601 keeps
// its standing definition: the Y entries exactly 0 (its luma weights ARE
// RGBToYIQ's) and nv12_chroma_matrix's I and Q (six-digit decode).
static inline void ycbcr_matrix(int fmt, double m[6])
{
    if (!fmt_matrix(fmt)) {
        double q[4];
        nv12_chroma_matrix(q);
        m[0] = m[3] = 0.0;
        m[1] = q[0], m[2] = q[1], m[4] = q[2], m[5] = q[3];
        return;
    }
    double kr, kb;
    matrix_krkb(fmt, &kr, &kb);
    const double kg = 1.0 - kr - kb;
    const double yiq[3][3] = {{0.299, 0.587, 0.114}, {0.596, -0.274, -0.322}, {0.211, -0.523, 0.312}};
    const double rgb_cb[3] = {0.0, -2.0 * kb * (1.0 - kb) / kg, 2.0 * (1.0 - kb)};
    const double rgb_cr[3] = {2.0 * (1.0 - kr), -2.0 * kr * (1.0 - kr) / kg, 0.0};
    for (int q = 0; q < 3; ++q) {
        m[q] = m[3 + q] = 0.0;
        for (int c = 0; c < 3; ++c) {
            m[q] += yiq[q][c] * rgb_cb[c];
            m[3 + q] += yiq[q][c] * rgb_cr[c];
        }
    }
}
static inline void nv12_chroma_matrix(double m[4])
{
    const double yiq[2][3] = {{0.596, -0.274, -0.322}, {0.211, -0.523, 0.312}};
    const double rgb_cb[3] = {0.0, -0.344136, 1.772}, rgb_cr[3] = {1.402, -0.714136, 0.0};
    for (int q = 0; q < 2; ++q) {
        m[q] = m[2 + q] = 0.0;
        for (int c = 0; c < 3; ++c) {
            m[q] += yiq[q][c] * rgb_cb[c];
            m[2 + q] += yiq[q][c] * rgb_cr[c];
        }
    }
}
// The launch geometry for frames of `fmt`: the handle's, the two sides'
// layouts, plus the NV12 range's
// scales and offsets (limited: Y 16 .. 235, C 16 .. 240; full: 0 .. 255) or
// the P010 range's (limited: Y 64 .. 940, C 64 .. 960; full: 0 .. 1023; the
// input side in units of the 16-bit word, 64 per code: u = 64).
static inline Geo geo_of(const mm_handle *h, const Frames &fr)
{
    if (fr.mixed()) {
        // each side's uniforms from its own format: the input-side fields
        // (y_off .. qcr, li.yb) of the in format's geometry, the output-side
        // fields (kr .. cro, lo.yb) of the out format's
        Frames a = fr, b = fr;
        a.ofmt = fr.fmt, a.fo = fr.fi;
        b.fmt = fr.ofmt, b.fi = fr.fo;
        Geo g = geo_of(h, a);
        const Geo go = geo_of(h, b);
        g.nv.kr = go.nv.kr, g.nv.kg = go.nv.kg, g.nv.kb = go.nv.kb;
        g.nv.yo_scale = go.nv.yo_scale, g.nv.yo_bias = go.nv.yo_bias;
        g.nv.cbo = go.nv.cbo, g.nv.cro = go.nv.cro;
        g.lo.yb = go.lo.yb;
        return g;
    }
    Geo g = h->geo;
    const int fmt = fr.fmt;
    const FmtInfo &f = *fr.fi;
    g.li = fr.in;
    g.lo = fr.out;
    // the order uniform, the same on both sides.  Packed 4:2:2: YUY2 is Y0 Cb
    // Y1 Cr (0), UYVY Cb Y0 Cr Y1 (1).  Packed RGB: 0: R G B, 1: B G R; K1's dot
    // weights and the compose kernels' byte selectors derive from it.
    g.li.yb = g.lo.yb = f.order | (fmt & f.opt & MM_ORDER_BGR ? 1u : 0u);
    if (f.ycc()) {
        // (MM_Y210: P010's words; MM_I010: its codes in the words' low bits, u = 1)
        const auto [ys, cs, y0, u] = code_range(f, f.full(fmt));
        double m[6], kr, kb;
        ycbcr_matrix(fmt, m);
        matrix_krkb(fmt, &kr, &kb);
        g.nv.y_off = (float)(y0 * u);
        g.nv.y_unit = (float)(1.0 / (ys * u));
        // K1 adds la (Cb - mid) + lb (Cr - mid) to (Y - y_off) before y_unit
        // scales the sum: Yq's a, b over the chroma scale, times the luma scale
        g.nv.la = (float)(m[0] * ys / cs);
        g.nv.lb = (float)(m[3] * ys / cs);
        g.nv.icb = (float)(m[1] / (cs * u));
        g.nv.qcb = (float)(m[2] / (cs * u));
        g.nv.icr = (float)(m[4] / (cs * u));
        g.nv.qcr = (float)(m[5] / (cs * u));
        g.nv.kr = (float)kr;
        g.nv.kg = (float)(1.0 - kr - kb);
        g.nv.kb = (float)kb;
        g.nv.yo_scale = (float)ys;
        g.nv.yo_bias = (float)(y0 + 0.5);
        // C' = (B - Yl) 0.5 / (1 - Kb), (R - Yl) 0.5 / (1 - Kr) (BT.601: 0.886,
        // 0.701); the mean of four; the code scale
        // (packed 4:2:2: the mean of the macropixel's two)
        g.nv.cbo = (float)(f.mean * cs * 0.5 / (1.0 - kb));
        g.nv.cro = (float)(f.mean * cs * 0.5 / (1.0 - kr));
    } else if (f.kfmt == kFmtY8 || f.kfmt == kFmtY16) {
        // v = sample / max in, code = floor(v max + 0.5) clamped to max out:
        // K1 runs the luma-plane instances (no offset), the compose instances
        // read the scale (also their clamp) and the rounding bias
        const double mx = (double)f.max;
        g.nv.y_off = 0.0f;
        g.nv.y_unit = (float)(1.0 / mx);
        g.nv.yo_scale = (float)mx;
        g.nv.yo_bias = 0.5f;
    }
    return g;
}

// ------------------------------------------------------------------------
// host tables
// ------------------------------------------------------------------------
static int wrap_host(int i, int n, int edge)
{
    if (edge) return i < 0 ? 0 : (i >= n ? n - 1 : i);
    int r = i % n;
    return r < 0 ? r + n : r;
}

static int next_pow2(int v)
{
    int n = 1;
    while (n < v) n <<= 1;
    return n;
}

// Composite of the stretch blit (src S texels -> N, RGBToYIQ pass, .cs:147) and
// the PadTexture quad resample (N -> S texels placed at (N-S)/2, .cs:358-381),
// both bilinear at texel t = u*size - 0.5, times the Hann window of the canvas
// position (WindowingFunction.shader:47-70).  fp32 formulas as the oracle.
static void build_tab(int S, int N, int edge, std::vector<Tap4> &tab)
{
    tab.resize(S);
    const int off = (N - S) / 2;
    for (int i = 0; i < S; ++i) {
        const int X = off + i;
        const float u = (float)(2 * X + 1 - (N - S)) / (float)(2 * S);
        const float tp = u * (float)N - 0.5f;
        const float af = floorf(tp);
        const int a = (int)af;
        const float gfr = tp - af;
        Tap4 e;
        for (int k = 0; k < 2; ++k) {
            const int aa = wrap_host(a + k, N, edge);
            const float us = ((float)aa + 0.5f) / (float)N;
            const float ts = us * (float)S - 0.5f;
            const float bf = floorf(ts);
            const int b = (int)bf;
            const float fr = ts - bf;
            const float wk = k ? gfr : 1.0f - gfr;
            // source indices stay UNWRAPPED (always in {i-1, i, i+1}); kernels wrap
            // them with the edge mode on use (wrap_near)
            e.idx[2 * k] = b;
            e.w[2 * k] = wk * (1.0f - fr);
            e.idx[2 * k + 1] = b + 1;
            e.w[2 * k + 1] = wk * fr;
        }
        const float wu = ((float)X + 0.5f) / (float)N;
        const float hann = 0.5f * (1.0f - cosf(2.0f * kPi * wu));
        for (int m = 0; m < 4; ++m) {
            e.w[m] *= hann;
            if (e.w[m] == 0.0f) e.idx[m] = i;   // zero taps (e.g. W == N) stay local
        }
        tab[i] = e;
    }
}

static void build_spec(const mm_params &p, int N, Spec &sp)
{
    memset(&sp, 0, sizeof(sp));
    sp.mode = p.mode;
    // standard mode: ProcessPhaseDifferenceWithComputeShader uniforms (.cs:489-506)
    sp.bp_apply = p.apply_bandpass_filter ? 1 : 0;
    sp.bp_low = p.low_frequency_cutoff;
    sp.bp_high = p.high_frequency_cutoff;
    sp.bp_steep = p.filter_steepness;
    sp.bp_sens = p.motion_sensitivity;
    sp.bp_edge = p.enhance_edges ? p.edge_enhancement : 0.0f;      // .cs:504
    sp.bp_inv_low = 1.0f / fmaxf(p.low_frequency_cutoff, 0.001f);
    sp.bp_inv_1mhigh = 1.0f / fmaxf(1.0f - p.high_frequency_cutoff, 0.001f);
    sp.bp_inv_band = 1.0f / (p.high_frequency_cutoff - p.low_frequency_cutoff);
    sp.L = p.levels;
    sp.minF = p.min_freq;
    sp.maxF = p.max_freq;
    sp.S = p.phase_scale;
    sp.tau2 = p.magnitude_threshold * p.magnitude_threshold;
    sp.inv_nn = 1.0f / ((float)N * (float)N);
    sp.S_rev = (float)((double)p.phase_scale / (2.0 * 3.14159265358979323846));
    sp.tau2_nn = sp.tau2 * sp.inv_nn * sp.inv_nn;   // exact: inv_nn is a power of two
    sp.hp_lo = p.max_freq * 0.8f;             // PyramidOperations.compute:36-41
    sp.hp_inv = 1.0f / (p.max_freq * 0.2f);
    sp.lp_hi = p.min_freq * 1.2f;             // PyramidOperations.compute:48-53
    sp.lp_inv = 1.0f / (p.min_freq * 0.2f);
    // steerable extension (mm_steer.hpp)
    sp.O = p.mode == MM_MODE_STEERABLE ? p.orientations : 1;
    sp.filt = p.temporal_filter;
    sp.r_low = p.iir_low;
    sp.r_high = p.iir_high;
    for (int k = 0; k < 8; ++k) {
        const double a = k < sp.O ? 2.0 * M_PI * k / sp.O : 0.0;
        sp.ang_c[k] = (float)cos(a);
        sp.ang_s[k] = (float)sin(a);
    }
    for (int i = 1; i < p.levels - 1; ++i) {
        // PyramidOperations.compute:59-64 (L=3: 0/0 = NaN -> empty band)
        volatile float num = (float)(i - 1), den = (float)(p.levels - 3);
        const float ratio = num / den;
        const float center = p.min_freq * powf(p.max_freq / p.min_freq, 1.0f - ratio);
        const float bwid = center * 0.5f;
        sp.lo[i] = center - bwid;
        sp.hi[i] = center + bwid;
        sp.inv_w[i] = 1.0f / (sp.hi[i] - sp.lo[i]);
    }
}

// k_cols' pyramid table holds <= 2 middle-band masks per bin: true unless some
// three bands share an open interval (ratio maxF/minF spread over few levels).
static bool bands_fit_table(const Spec &sp)
{
    for (int a = 1; a < sp.L - 1; ++a)
        for (int b = a + 1; b < sp.L - 1; ++b)
            for (int c = b + 1; c < sp.L - 1; ++c) {
                const float lo = fmaxf(sp.lo[a], fmaxf(sp.lo[b], sp.lo[c]));
                const float hi = fminf(sp.hi[a], fminf(sp.hi[b], sp.hi[c]));
                if (lo < hi) return false;   // NaN bands (L = 3) compare false
            }
    return true;
}

// The tabled ops take the phase of p conj c, which is 0 for an exactly zero p
// or c; the reference takes arg p - arg c with atan2(0, 0) = 0, that is -arg c
// for a zero p.  A positive threshold gates every such bin (0 < tau^2 / N^4);
// where it cannot (magnitude_threshold = 0, or one whose scaled square
// underflows), K2 runs the generic op, which handles the zero bins.
static bool tau_gates_zero_bins(const Spec &sp)
{
    return sp.tau2_nn >= 1.17549435e-38f;
}

// Two middle bands overlap on an interval of positive width (relative 1e-5:
// bands that only touch at a mask zero, L <= 5 at the default 0.05 / 0.45,
// can share a bin by a rounding ulp, which the kernel's per-wave check still
// routes to the generic op): k_cols runs MM_K2_PYR_TAB2.
static bool bands_overlap(const Spec &sp)
{
    for (int a = 1; a < sp.L - 1; ++a)
        for (int b = a + 1; b < sp.L - 1; ++b) {
            const float lo = fmaxf(sp.lo[a], sp.lo[b]), hi = fminf(sp.hi[a], sp.hi[b]);
            if (hi - lo > 1e-5f * hi) return true;   // NaN bands (L = 3) compare false
        }
    return false;
}

// GaussianBlur.shader:47-60 at _BlurSize 0.5 (.cs:427): bilinear taps at
// +-0.6923 and +-1.6154 texels == a 5-tap FIR.
static Blur5 build_blur()
{
    const double c0 = 0.2270270270, c1 = 0.3162162162, c2w = 0.0702702703;
    const double f1 = 0.5 * 1.3846153846, f2 = 0.5 * 3.2307692308 - 1.0;
    const double w0 = c0 + 2.0 * c1 * (1.0 - f1), w1 = c1 * f1 + c2w * (1.0 - f2), w2 = c2w * f2;
    Blur5 b;
    b.w0 = (float)w0;
    b.w1 = (float)w1;
    b.w2 = (float)w2;
    // the RGBA8 compose's vertical blur in code units (yiq_rgba8): 255 x, rounded once
    b.c0 = (float)(255.0 * w0);
    b.c1 = (float)(255.0 * w1);
    b.c2 = (float)(255.0 * w2);
    return b;
}

static int validate_params(const mm_params *p)
{
    if (!p) return MM_ERR_INVALID;
    if (p->levels < 1 || p->levels > kMaxLevels) return MM_ERR_UNSUPPORTED;
    if (p->mode == MM_MODE_STEERABLE) {
        // cos^4 lobes cover every direction from 4 orientations up; even O pairs
        // each lobe with its conjugate mirror (oracle/steerable_ref.py)
        if (p->orientations != 4 && p->orientations != 6 && p->orientations != 8)
            return MM_ERR_UNSUPPORTED;
        if (p->temporal_filter != MM_FILTER_DIFF && p->temporal_filter != MM_FILTER_IIR)
            return MM_ERR_INVALID;
        if (p->temporal_filter == MM_FILTER_IIR &&
            !(p->iir_low > 0.0f && p->iir_low < p->iir_high && p->iir_high <= 1.0f))
            return MM_ERR_INVALID;
    } else {
        if (p->orientations != 1) return MM_ERR_UNSUPPORTED;
        if (p->mode != MM_MODE_PYRAMID && p->mode != MM_MODE_STANDARD) return MM_ERR_UNSUPPORTED;
    }
    if (p->edge_mode != MM_EDGE_REPEAT && p->edge_mode != MM_EDGE_CLAMP) return MM_ERR_INVALID;
    if (!(p->min_freq > 0.0f) || !(p->max_freq > 0.0f)) return MM_ERR_INVALID;
    return MM_OK;
}

// ------------------------------------------------------------------------
// launches
// ------------------------------------------------------------------------
// slots of one column of K2's per-bin table (k2_tab_slots)
static constexpr int ktab_slots(int log2n)
{
    const int C = fft_c_v(log2n), te = (1 << log2n) / 2 + 1;
    return (te + C - 1) / C * C;
}

static int ilog2(int n)
{
    int l = 0;
    while ((1 << l) < n) ++l;
    return l;
}

template <int LOG2N> static size_t lds_fft_bytes()
{
    return sizeof(c2) * (size_t)groups_per_wg<LOG2N>() * lds_complex<(1 << LOG2N)>();
}
// k_rows_inv_compose's dynamic LDS: two FFT regions, and in front of them the
// four staged source rows of the SRCDMA instances (the launch and set_attrs)
template <int LOG2N> static size_t k34_lds_bytes(bool srcdma)
{
    return sizeof(c2) * 2 * lds_complex<(1 << LOG2N)>() + (srcdma ? (size_t)k34_src_bytes<LOG2N>() : 0);
}
template <int LOG2N>
static int set_attrs(int W)
{
    (void)W;   // every other kernel stays within the default 64 KiB dynamic LDS
    // k_rows_inv_compose with staged source rows: 68.9 KB at N = 2048, 137.7 KB at N = 4096
    if constexpr (LOG2N <= 12) if (k34_lds_bytes<LOG2N>(true) > 65536) {
        const int lds = (int)k34_lds_bytes<LOG2N>(true);
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rows_inv_compose<LOG2N, MM_RGBA8, true>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rows_inv_compose<LOG2N, MM_RGBA8_SRGB, true>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rows_inv_compose<LOG2N, kFmtRGBA8toNV12, true>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rows_inv_compose<LOG2N, kFmtBGRA8, true>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rows_inv_compose<LOG2N, kFmtBGRA8S, true>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rows_inv_compose<LOG2N, kFmtBGRA8toNV12, true>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    }
    if constexpr (LOG2N == 12) {   // k_rows_inv_compose: two 4096-point groups, 73.7 KB
        const int lds = (int)k34_lds_bytes<12>(false);
        for (int f : {MM_RGBA8, MM_RGBA32F, MM_RGBA16F, MM_RGBA8_SRGB, MM_NV12, MM_P010, MM_Y8, MM_Y16, MM_YUY2, MM_Y210, MM_RGB24, MM_I420, MM_I010, MM_BGRA8, MM_BGRA8_SRGB})
            MM_FMT_SWITCH(fmt_info(f), HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rows_inv_compose<12, FMT_>),
                                                        hipFuncAttributeMaxDynamicSharedMemorySize, lds)))
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rows_inv_compose<12, kFmtNV12toRGBA8>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rows_inv_compose<12, kFmtP010toRGBA8>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rows_inv_compose<12, kFmtRGBA8toNV12>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rows_inv_compose<12, kFmtNV12toBGRA8>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rows_inv_compose<12, kFmtP010toBGRA8>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rows_inv_compose<12, kFmtBGRA8toNV12>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        // k_sb_cols: exchange buffer (36.9 KB) + its own staging, past 64 KB for
        // frames taller than ~3,570 rows (run_steer's bound)
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_sb_cols<12>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 81920));
    }
    if constexpr (LOG2N == 13) {   // N = 8192: one 8192-point transform per workgroup, 73.7 KB and more
        auto set = [](const void *f, size_t b) {
            return b > 65536 ? hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b)
                             : hipSuccess;
        };
        const size_t x = sizeof(c2) * lds_complex<8192>();
        HIPCHK(set(reinterpret_cast<const void *>(&k_rows_inv<13>), sizeof(c2) * k3_groups<13>() * lds_complex<8192>()));
        HIPCHK(set(reinterpret_cast<const void *>(&k_dbg_cols<13>), 2 * sizeof(c2) * lds_complex<4096>()));
        (void)x;
#define MM_SET_K2(MODE)                                                                                  \
        HIPCHK(set(reinterpret_cast<const void *>(&k_cols<13, MODE>), k2_lds_bytes<13, MODE>()));        \
        HIPCHK(set(reinterpret_cast<const void *>(&k_cols_tail<13, MODE>), k2_lds_bytes<13, MODE>()));   \
        HIPCHK(set(reinterpret_cast<const void *>(&k_cols_hold<13, MODE>), k2_lds_bytes<13, MODE>()));   \
        HIPCHK(set(reinterpret_cast<const void *>(&k_cols_tail_hold<13, MODE>), k2_lds_bytes<13, MODE>()))
        MM_SET_K2(MM_MODE_PYRAMID);
        MM_SET_K2(MM_MODE_STANDARD);
        MM_SET_K2(MM_K2_PYR_TAB);
        // (no two-band instance: its mask-sum arrays would take K2 past 160 KB
        // of LDS at N = 8192; overlapping bands run the generic op there)
#undef MM_SET_K2
    }
    if constexpr (LOG2N == 11) {   // k_rows_inv_compose4: four 2048-point groups, 73.7 KB
        const int lds = (int)(sizeof(c2) * 4 * lds_complex<2048>());
        for (int f : {MM_RGBA8, MM_RGBA32F, MM_RGBA16F, MM_RGBA8_SRGB, MM_NV12, MM_P010, MM_Y8, MM_Y16, MM_YUY2, MM_Y210, MM_RGB24, MM_I420, MM_I010, MM_BGRA8, MM_BGRA8_SRGB})
            MM_FMT_SWITCH(fmt_info(f), HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rows_inv_compose4<11, FMT_>),
                                                        hipFuncAttributeMaxDynamicSharedMemorySize, lds)))
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rows_inv_compose4<11, kFmtNV12toRGBA8>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rows_inv_compose4<11, kFmtP010toRGBA8>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rows_inv_compose4<11, kFmtRGBA8toNV12>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rows_inv_compose4<11, kFmtNV12toBGRA8>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rows_inv_compose4<11, kFmtP010toBGRA8>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rows_inv_compose4<11, kFmtBGRA8toNV12>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    }
    return MM_OK;
}

template <int LOG2N>
static int launch_k1(mm_handle *h, const uint8_t *in, int nframes, const Frames &fr, hipStream_t s, c2 *G)
{
    const int ppf = (h->H + 1) / 2;   // odd H: the last pair's second row is zero
    const int total = ppf * nframes;
    // fewer than 2 workgroups per CU at the batch form: the one-pair form
    const bool lat = (total + k1_groups<LOG2N>() - 1) / k1_groups<LOG2N>() < 512;
    ProfScope ps(h, s, MM_K_ROWS_FWD, nframes);
#define MM_K1_LAUNCH(F, GEN, LAT)                                                                  \
    do {                                                                                           \
        constexpr int gpw = k1_gpw<LOG2N, LAT>();                                                  \
        const size_t lds = sizeof(c2) * (size_t)gpw * lds_complex<(1 << LOG2N)>();                \
        if (lds > 65536)                                                                           \
            HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rows_fwd<LOG2N, F, GEN, LAT>), \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));     \
        hipLaunchKernelGGL((k_rows_fwd<LOG2N, F, GEN, LAT>), dim3((total + gpw - 1) / gpw),         \
                           dim3(gpw * fft_T<LOG2N>()), lds, s, in, ppf, total, g,                  \
                           h->d_col3, h->d_row3, h->d_col, h->d_row, h->d_tw, G, h->g_stride);     \
    } while (0)
    const bool gen = h->geo.ox || h->geo.oy;   // odd W/H: taps span i-2 .. i+1
    const Geo g = geo_of(h, fr);
    if (gen) {   // (4:2:0 frames have even sizes; single-plane ones run the luma-plane instances here too)
        MM_FMT_SWITCH_FULLRES(fr.fi, MM_K1_LAUNCH(kK1Fmt<FMT_>, true, false))
    } else {
        MM_FMT_SWITCH_K1(fr.fi, fr.fmt, if (lat) MM_K1_LAUNCH(kK1Fmt<FMT_>, false, true);
                              else MM_K1_LAUNCH(kK1Fmt<FMT_>, false, false))
    }
#undef MM_K1_LAUNCH
    HIPCHK(hipGetLastError());
    return MM_OK;
}

// K2's per-bin tables, stream-ordered before the K2 launch that follows a
// parameter change
template <int LOG2N>
static int refresh_k2_tables(mm_handle *h, hipStream_t s)
{
    const int cols = (1 << LOG2N) / 2;
    static_assert(ktab_slots(LOG2N) == k2_tab_slots<LOG2N>(), "d_ktab column stride");
    const int tab_mode = h->spec.mode == MM_MODE_STANDARD ? MM_MODE_STANDARD : h->k2_tab ? MM_K2_PYR_TAB : -1;
    if (tab_mode >= 0 && h->ktab_mode != tab_mode) {
        const int n = (cols + 1) * k2_tab_slots<LOG2N>();
        if (tab_mode == MM_MODE_STANDARD)
            hipLaunchKernelGGL((k_k2_table<LOG2N, MM_MODE_STANDARD>), dim3((n + 255) / 256), dim3(256), 0, s,
                               h->d_ktab, h->d_kmsum, h->spec);
        else
            hipLaunchKernelGGL((k_k2_table<LOG2N, MM_K2_PYR_TAB>), dim3((n + 255) / 256), dim3(256), 0, s,
                               h->d_ktab, h->d_kmsum, h->spec);
        HIPCHK(hipGetLastError());
        h->ktab_mode = tab_mode;
    }
    return MM_OK;
}

// K2 over frames G[0 .. nframes) (K1's row spectra), primed with Gprev = G_{t-1}
// (the state slot, or frame 0 itself for a stream's first batch, whose frame 0
// passes through): Q of frame fr to d_Q + fr * q_stride.
// hold: every frame pairs with Gprev (k_cols_hold, k_cols_tail_hold; the same
// tail split).  One frame rolls nothing: it keeps the rolling instance.
template <int LOG2N>
static int launch_k2(mm_handle *h, int nframes, const c2 *Gprev, const c2 *G, hipStream_t s, bool hold = false)
{
    hold = hold && nframes >= 2;
    const int gpw = k2_groups<LOG2N>();
    const int cols = (1 << LOG2N) / 2;   // f = 0 and f = N/2 share group 0 (k_cols)
    const int blocks = (cols + gpw - 1) / gpw;
    if (int rc = refresh_k2_tables<LOG2N>(h, s)) return rc;
    ProfScope ps(h, s, MM_K_COLS, nframes);
    // the packed block's last k frames go to k_cols_tail (k_cols's critical path)
    int k = nframes >= 24 ? nframes * h->k2_tail_pct / 100 : 0;
    k = std::max(0, std::min(k, nframes - 2));
    // second-half tails (k_cols): the last k2 frames of each second-half block's
    // columns in extra blocks (MM_K2_TAIL2 percent)
    const int k2t = nframes >= 24 && blocks >= 2 ? std::min(nframes * h->k2_tail2_pct / 100, nframes - 2) : 0;
    const int tb = k2t > 0 ? blocks / 2 : 0;
#define MM_K2_LAUNCH_(MODE, COLS, TAIL)                                                              \
    do {                                                                                             \
        /* exchange buffers + per-bin tables + the packed group's */                                 \
        const size_t lds = k2_lds_bytes<LOG2N, MODE>();                                              \
        hipLaunchKernelGGL((COLS<LOG2N, MODE>), dim3(blocks + tb), dim3(k2_threads<LOG2N>()), lds, s, G, \
                           h->g_stride, Gprev, h->d_Q, h->q_stride, nframes, h->geo, h->spec, h->d_tw, h->d_ktab, \
                           h->d_kmsum, nframes - k, tb, k2t);                                        \
        if (k)                                                                                       \
            hipLaunchKernelGGL((TAIL<LOG2N, MODE>), dim3(k), dim3(k2_threads<LOG2N>()), lds, s, G,   \
                               h->g_stride, Gprev, h->d_Q, h->q_stride, nframes - k, h->geo, h->spec, h->d_tw, \
                               h->d_ktab, h->d_kmsum);                                               \
    } while (0)
#define MM_K2_LAUNCH(MODE)                                                                           \
    do {                                                                                             \
        if (hold) MM_K2_LAUNCH_(MODE, k_cols_hold, k_cols_tail_hold);                                \
        else MM_K2_LAUNCH_(MODE, k_cols, k_cols_tail);                                               \
    } while (0)
    if (h->spec.mode == MM_MODE_STANDARD) MM_K2_LAUNCH(MM_MODE_STANDARD);
    else if (h->k2_tab2) MM_K2_LAUNCH(MM_K2_PYR_TAB2);
    else if (h->k2_tab) MM_K2_LAUNCH(MM_K2_PYR_TAB);
    else MM_K2_LAUNCH(MM_MODE_PYRAMID);
#undef MM_K2_LAUNCH
#undef MM_K2_LAUNCH_
    HIPCHK(hipGetLastError());
    return MM_OK;
}

// K2 of one frame of each lane of `sel`: lane k's G_{t-1} in slot k of the
// bank that bit k of `banks` names, its G_t in the other bank's slot k, its Q
// to d_LQ + k * q_stride.  One launch, whatever the mask and the bank bits:
// k_cols_lanes where every lane is selected and all have one bank bit (every
// call of a handle that only gets full calls), k_cols_lanes_sel otherwise.
// The modes and their order are launch_k2's.
template <int LOG2N>
static int launch_k2_lanes(mm_handle *h, uint64_t sel, uint64_t banks, hipStream_t s)
{
    const int gpw = k2_groups<LOG2N>();
    const int blocks = ((1 << LOG2N) / 2 + gpw - 1) / gpw;
    const int nsel = __builtin_popcountll(sel);
    const uint64_t all = h->lanes >= 64 ? ~0ull : (1ull << h->lanes) - 1;
    const bool plain = sel == all && ((banks & all) == 0 || (banks & all) == all);
    const size_t bank = h->g_stride * (size_t)h->lanes;
    const c2 *Gprev = h->d_LG + bank * (banks & 1), *G = h->d_LG + bank * (1 - (banks & 1));   // (plain)
    if (int rc = refresh_k2_tables<LOG2N>(h, s)) return rc;
    ProfScope ps(h, s, MM_K_COLS, nsel);
#define MM_K2_LAUNCH(MODE)                                                                           \
    do {                                                                                             \
        const size_t lds = k2_lds_bytes<LOG2N, MODE>();                                              \
        if (plain)                                                                                   \
            hipLaunchKernelGGL((k_cols_lanes<LOG2N, MODE>), dim3(blocks, h->lanes), dim3(k2_threads<LOG2N>()), lds, s, \
                               G, h->g_stride, Gprev, h->d_LQ, h->q_stride, h->geo, h->spec, h->d_tw, h->d_ktab, \
                               h->d_kmsum);                                                          \
        else                                                                                         \
            hipLaunchKernelGGL((k_cols_lanes_sel<LOG2N, MODE>), dim3(blocks, nsel), dim3(k2_threads<LOG2N>()), lds, s, \
                               h->d_LG, h->g_stride, h->d_LQ, h->q_stride, (unsigned long long)sel,  \
                               (unsigned long long)banks, h->lanes, h->geo, h->spec, h->d_tw, h->d_ktab, \
                               h->d_kmsum);                                                          \
    } while (0)
    if (h->spec.mode == MM_MODE_STANDARD) MM_K2_LAUNCH(MM_MODE_STANDARD);
    else if (h->k2_tab2) MM_K2_LAUNCH(MM_K2_PYR_TAB2);
    else if (h->k2_tab) MM_K2_LAUNCH(MM_K2_PYR_TAB);
    else MM_K2_LAUNCH(MM_MODE_PYRAMID);
#undef MM_K2_LAUNCH
    HIPCHK(hipGetLastError());
    return MM_OK;
}

// Grows a per-batch buffer that only some paths use to `frames` frames of
// `per_frame` bytes.  The old buffer is retired behind this handle's work
// (its previous calls and what this call queued on s), not behind the
// device's; a failed allocation leaves the old one in place.
static int ensure_frames(mm_handle *h, void **buf, int *have, int frames, size_t per_frame, hipStream_t s)
{
    if (*buf && *have >= frames) return MM_OK;
    void *p = nullptr;
    if (h_alloc(h, &p, per_frame * (size_t)frames) != hipSuccess) return MM_ERR_OOM;
    h_retire(h, *buf, s, true);
    *buf = p;
    *have = frames;
    return MM_OK;
}
static int ensure_yh(mm_handle *h, hipStream_t s)
{
    // (a batch's frames, or a lane call's)
    return ensure_frames(h, reinterpret_cast<void **>(&h->d_Yh), &h->yh_frames, std::max(h->chunk, h->lanes),
                         sizeof(float) * h->yh_stride, s);
}

// G slot of the first frame of an n-frame batch: the batch must not
// overwrite the state slot gs (read by the batch's K2 as G_{t-1}).  With
// chunk + 1 slots the state moves (one slot copy) only when neither the slots
// after gs nor those before it hold the batch: once per full batch at most,
// never in the one-frame-per-call pattern (it alternates slots 0 and 1).
static int place_batch(mm_handle *h, int n, hipStream_t s, int *base)
{
    *base = 0;
    if (!h->g_valid) return MM_OK;   // no state slot to keep
    if (h->gs + 1 + n <= h->chunk + 1) {
        *base = h->gs + 1;
        return MM_OK;
    }
    if (n > h->gs) {
        HIPCHK(hipMemcpyAsync(h->d_G + h->g_stride * h->chunk, h->d_G + h->g_stride * h->gs,
                              sizeof(c2) * h->g_stride, hipMemcpyDeviceToDevice, s));
        h->gs = h->chunk;
    }
    return MM_OK;
}

static int launch_k4(mm_handle *h, const uint8_t *in, uint8_t *out, int frame0, int nframes,
                     const Frames &fr, hipStream_t s);

// Whether the row starts of `nframes` frames at p, layout l of format f, are
// multiples of a_luma (the first plane's) and a_chroma (the chroma planes').  A
// row start is a sum of the base, a plane offset, pitches, the Cr plane's
// distance from the Cb plane and, past one frame, frame strides (a stream
// whose frames are 2 mod 4 apart alternates alignment: decided for all its
// frames here, not from its first one): all of them multiples, so is every row.
static bool rows_aligned(const FmtInfo &f, const uint8_t *p, const Geo::Lay &l, int H, int nframes,
                         unsigned a_luma, unsigned a_chroma)
{
    const uintptr_t b = reinterpret_cast<uintptr_t>(p);
    uintptr_t luma = b | l.pitch, chroma = 0;
    if (f.planes > 1) chroma = (b + l.c_off) | l.c_pitch;
    if (f.planes > 2) chroma |= i420_cr_delta(H, l.c_pitch);
    if (nframes > 1) luma |= l.stride, chroma |= l.stride;
    return !(luma & (a_luma - 1)) && !(chroma & (a_chroma - 1));
}
// The RGBA8 and BGRA8 formats' source rows staged in LDS (k_rows_inv_compose<.., true>):
// a thread's quad travels as one 16-byte LDS-DMA, taken only where every quad
// of every source row of the launch is 16-byte aligned (X % 4 == 0).  Any other
// layout keeps the register loads, which need dword alignment only.  Same results.
static bool k34_src_dma(const mm_handle *h, const uint8_t *in, const Frames &fr, int nframes)
{
    // (a convert call with MM_RGBA8 or MM_BGRA8 in is the encode pair: the same source rows)
    return (fr.fmt == MM_RGBA8 || fr.fmt == MM_RGBA8_SRGB || fr.fmt == MM_BGRA8 || fr.fmt == MM_BGRA8_SRGB) &&
           rows_aligned(*fr.fi, in, fr.in, h->H, nframes, 16, 1);
}
// k_rows_inv_compose's layouts: quads at the alignment each side's format asks
// of its rows (FmtInfo::quad; a convert call: the input numbers of the input
// format, the output numbers of the output format) ...
static bool k34_quads_aligned(const mm_handle *h, const uint8_t *in, const uint8_t *out, const Frames &fr, int nframes)
{
    const uint8_t *qi = fr.fi->quad, *qo = fr.fo->quad;
    return rows_aligned(*fr.fi, in, fr.in, h->H, nframes, qi[0], qi[1]) &&
           rows_aligned(*fr.fo, out, fr.out, h->H, nframes, qo[2], qo[3]);
}
// ... and its geometry: even sizes whose quads tile the rows (W % 8 == 0
// puts x0 on a multiple of 4), the horizontal blur's float4 taps inside the
// canvas, and no vertical blur tap wrapping (list row of output row i + v is i + v)
static bool k34_fits(const mm_handle *h, const uint8_t *in, const uint8_t *out, const Frames &fr, int nframes)
{
    // a grouped format (v210: six pixels to a store unit) has no fused instance
    // in any form, the walking kernel, the one-shot and the lanes' alike
    if (fr.fi->grp_px || fr.fo->grp_px) return false;
    if (!k34_quads_aligned(h, in, out, fr, nframes)) return false;
    const Geo &g = h->geo;
    return g.N <= 4096 &&   // two transforms per workgroup: 2 N / 8 <= 1024 threads
           !g.ox && !g.oy && g.W % 8 == 0 && g.x0 >= 4 && g.x0 % 4 == 0 &&
           g.x0 + g.W + 4 <= g.N && g.N - g.H >= 4 && g.Hn == g.H + 4 && g.rb == g.y0 - 2 &&
           2 * (g.N / 8) >= g.W / 4;
}

// Strip height of one k_rows_inv_compose launch over nout frames.  A strip is
// one workgroup walking its rows in sequence, so a launch needs many strips:
// about 4 workgroups per CU (H nout / R >= 1024) with R <= 64, and the unfused
// pair (0) when that would take strips under 16 rows (the one-frame drop-in
// call: K3 + K4 spread one frame over thousands of workgroups).  MM_K34_ROWS
// forces a strip height (0: unfused).
#ifndef MM_K34_ROWS_4K
#define MM_K34_ROWS_4K 128
#endif
static int k34_strip_rows(const mm_handle *h, int nout)
{
    if (h->k34_rows >= 0) return h->k34_rows;
    // at N = 4096 a K34 workgroup (1,024 threads, 125 VGPRs) is alone on its
    // CU, so a longer strip halves the halo rows at no cost in concurrency
    // (C3 same-call: R 64 -> 128, K34 26.4-26.8 -> 25.7-25.8 us per frame;
    // at 1080p 96 and 128 were slower than 64)
    const int cap = h->N >= 4096 ? MM_K34_ROWS_4K : 64;
    const int R = std::min(cap, (int)((long long)h->H * nout / 1024) / 4 * 4);
    return R >= 16 ? R : 0;
}

// K3 + K4 of frames [frame0, nframes) whose Q lie at Q + frame * q_stride
// (a batch's d_Q, or the lanes' d_LQ)
template <int LOG2N>
static int launch_k3(mm_handle *h, const c2 *Q, const uint8_t *in, uint8_t *out, int frame0, int nframes,
                     const Frames &fr, hipStream_t s)
{
    const int nout = nframes - frame0;
    if (nout <= 0) return MM_OK;
    const int fmt = fr.fmt;
    const int R = k34_strip_rows(h, nout);
    // Short launches (the one-frame call) at N <= 1024 whose strips fit one
    // workgroup round (4 waves per SIMD at <= 128 VGPRs: 1024 / 4T workgroups
    // per CU): K3 + K4 fused in one shot, four FFT groups per 4-row strip, no
    // walk (k_rows_inv_compose4).  One-frame calls, same call
    // (profiles/r03k_k34_oneshot.txt): 960x540 33.0 -> 29.8 us, 640x480
    // 30.4 -> 28.3 us, 1024x768 equal; at N = 2048 (16-wave workgroups, one
    // per CU) it lost even in one round (1280x720 42.0 -> 42.6 us) and 1080p's
    // 270 strips take two rounds (48.0 -> 54.4 us): K3 -> K4 there
    // (MM_K34_ONESHOT=2 forces it, 0 disables it).
    constexpr int k34o_per_cu = 4 * fft_T<LOG2N>() <= 1024 ? 1024 / (4 * fft_T<LOG2N>()) : 0;
    if constexpr (LOG2N <= 11) if (R == 0 && h->k34_rows < 0 && h->k34_oneshot && k34_fits(h, in, out, fr, nframes) &&
                                   ((LOG2N <= 10 && (h->H + 3) / 4 * nout <= k34o_per_cu * h->num_cu) ||
                                    h->k34_oneshot == 2)) {
        const int strips = (h->H + 3) / 4;
        const size_t lds = sizeof(c2) * 4 * lds_complex<(1 << LOG2N)>();
        const dim3 grid((unsigned)(strips * nout)), block(4 * fft_T<LOG2N>());
        ProfScope ps(h, s, MM_K_ROWS_INV_COMPOSE, nout);
        MM_PAIR_SWITCH(fr, hipLaunchKernelGGL((k_rows_inv_compose4<LOG2N, FMT_>), grid, block, lds, s, Q,
                                              h->q_stride, in, out, frame0, strips, geo_of(h, fr), h->blur,
                                              h->d_col3, h->d_row3, h->d_tw))
        HIPCHK(hipGetLastError());
        return MM_OK;
    }
    if (R >= 4 && k34_fits(h, in, out, fr, nframes)) {   // K3 + K4 fused: Yh stays on chip
        const int strips = (h->H + R - 1) / R, steps = R / 4 + 1;
        const bool dma = LOG2N <= 12 && k34_src_dma(h, in, fr, nframes);
        const size_t lds = k34_lds_bytes<LOG2N>(dma);
        const dim3 grid((unsigned)(strips * nout)), block(2 * fft_T<LOG2N>());
        ProfScope ps(h, s, MM_K_ROWS_INV_COMPOSE, nout);
#define MM_K34_LAUNCH(F, DMA)                                                                        \
        hipLaunchKernelGGL((k_rows_inv_compose<LOG2N, F, DMA>), grid, block, lds, s, Q,               \
                           h->q_stride, in, out, frame0, strips, steps, geo_of(h, fr), h->blur,      \
                           h->d_col3, h->d_row3, h->d_tw)
        if constexpr (LOG2N <= 12) if (dma) {
            if (fr.mixed() && fmt == MM_BGRA8) MM_K34_LAUNCH(kFmtBGRA8toNV12, true);
            else if (fr.mixed()) MM_K34_LAUNCH(kFmtRGBA8toNV12, true);
            else if (fmt == MM_RGBA8) MM_K34_LAUNCH(MM_RGBA8, true);
            else if (fmt == MM_BGRA8) MM_K34_LAUNCH(kFmtBGRA8, true);
            else if (fmt == MM_BGRA8_SRGB) MM_K34_LAUNCH(kFmtBGRA8S, true);
            else MM_K34_LAUNCH(MM_RGBA8_SRGB, true);
        }
        if (!dma) MM_PAIR_SWITCH(fr, MM_K34_LAUNCH(FMT_, false))
#undef MM_K34_LAUNCH
        HIPCHK(hipGetLastError());
        return MM_OK;
    }
    const int ppf = h->geo.Hq / 2;   // whole Q tiles (k_rows_inv)
    const int total = ppf * nout;
    const int gpw = k3_groups<LOG2N>();
    int rc = ensure_yh(h, s);
    if (rc) return rc;
    {
        ProfScope ps(h, s, MM_K_ROWS_INV, nout);
        hipLaunchKernelGGL((k_rows_inv<LOG2N>), dim3((total + gpw - 1) / gpw),
                           dim3(k3_threads<LOG2N>()), sizeof(c2) * (size_t)gpw * lds_complex<(1 << LOG2N)>(),
                           s, Q,
                           h->q_stride, h->d_Yh, h->yh_stride, frame0, ppf, total, h->geo,
                           h->blur, h->d_tw);
        HIPCHK(hipGetLastError());
    }
    return launch_k4(h, in, out, frame0, nframes, fr, s);
}

// k_compose's instance of a format (the single-plane formats': k_compose_mono)
template <int FMT> static constexpr auto k4_kernel()
{
    if constexpr (kMono<FMT>) return &k_compose_mono<FMT>;
    else return &k_compose<FMT>;
}
// K4 k_compose over chunk frames [frame0, nframes) (Yh of those frames ready)
static int launch_k4(mm_handle *h, const uint8_t *in, uint8_t *out, int frame0, int nframes,
                     const Frames &fr, hipStream_t s)
{
    const int nout = nframes - frame0;
    if (nout <= 0) return MM_OK;
    if (h->geo.ox || h->geo.oy) {   // odd W/H: the crop samples between texels
        const size_t tot = (size_t)nout * h->W * h->H;
        ProfScope ps(h, s, MM_K_COMPOSE, nout);
        const dim3 grid((unsigned)((tot + 255) / 256));
        MM_FMT_SWITCH_FULLRES(fr.fi, hipLaunchKernelGGL((k_compose_odd<FMT_>), grid, dim3(256), 0, s, h->d_Yh,
                                              h->yh_stride, in, out, frame0, nout, geo_of(h, fr), h->blur,
                                              h->d_col, h->d_row))
        HIPCHK(hipGetLastError());
        return MM_OK;
    }
    const int rt = (h->H + kTileRows - 1) / kTileRows, ct = (h->W + kTileCols - 1) / kTileCols;
    const dim3 grid(rt * ct * nout);
    ProfScope ps(h, s, MM_K_COMPOSE, nout);
    if (fr.fi->kfmt == kFmtV210) {   // column tiles of whole 6-pixel groups (no mixed pair has it)
        const int ctg = (h->W + kTileColsG - 1) / kTileColsG;
        hipLaunchKernelGGL((k_compose<kFmtV210>), dim3(rt * ctg * nout), dim3(k4_tile_cols<kFmtV210>), 0, s, h->d_Yh,
                           h->yh_stride, in, out, frame0, rt, ctg, geo_of(h, fr), h->blur, h->d_col3, h->d_row3);
        HIPCHK(hipGetLastError());
        return MM_OK;
    }
    MM_PAIR_SWITCH(fr, hipLaunchKernelGGL((k4_kernel<FMT_>()), grid, dim3(kTileCols), 0, s, h->d_Yh,
                                          h->yh_stride, in, out, frame0, rt, ct, geo_of(h, fr), h->blur,
                                          h->d_col3, h->d_row3))
    HIPCHK(hipGetLastError());
    return MM_OK;
}

// Passthrough of n frames (the first frame, apply_magnification = 0): the
// W x H samples bitwise, the destination's padding untouched.  Tight frames
// back to back on both sides are one device copy; any other layout goes
// through k_copy_rows, one launch for the n frames.
static int convert_frames(mm_handle *h, const uint8_t *in, uint8_t *out, int n, const Frames &fr, hipStream_t s);
static int copy_frames(mm_handle *h, const uint8_t *in, uint8_t *out, int n, const Frames &fr, hipStream_t s)
{
    if (n <= 0) return MM_OK;
    if (fr.mixed()) return convert_frames(h, in, out, n, fr, s);   // no bitwise passthrough between two formats
    if (fr.packed) {
        HIPCHK(hipMemcpyAsync(out, in, fr.fb * n, hipMemcpyDeviceToDevice, s));
        return MM_OK;
    }
    const FmtInfo &f = *fr.fi;
    const unsigned rb = (unsigned)f.row_bytes(h->W);
    const int rows = f.planes == 2 ? h->H + h->H / 2 : h->H;   // (a (Cb, Cr) plane: its rows after the luma rows)
    // in words of the format's unit: bytes, 16-bit words, or dwords, which divide every larger unit
    const auto copy = f.unit == 1 ? &k_copy_rows<uint8_t> : f.unit == 2 ? &k_copy_rows<uint16_t> : &k_copy_rows<uint32_t>;
    const Geo g = geo_of(h, fr);
    // three planes of row bytes W, W/2 and W/2: the luma rows, then the two
    // chroma planes as H/2 "luma" rows (Cb) and H/2 chroma rows (Cr) of a
    // geometry whose planes are the Cb and Cr planes
    Geo gc = g;
    if (f.planes == 3) {
        gc.li.pitch = g.li.c_pitch, gc.li.c_off = (unsigned)i420_cr_delta(h->H, g.li.c_pitch);
        gc.lo.pitch = g.lo.c_pitch, gc.lo.c_off = (unsigned)i420_cr_delta(h->H, g.lo.c_pitch);
    }
    for (int f0 = 0; f0 < n; f0 += 32768) {   // (grid y <= 65535)
        const dim3 grid((unsigned)rows, (unsigned)std::min(32768, n - f0));
        const uint8_t *src = in + fr.in.stride * f0;
        uint8_t *dst = out + fr.out.stride * f0;
        if (f.planes == 3) {
            const dim3 gy((unsigned)h->H, grid.y);   // H luma rows; H/2 Cb + H/2 Cr rows
            hipLaunchKernelGGL(copy, gy, dim3(256), 0, s, src, dst, g, rb, h->H);
            hipLaunchKernelGGL(copy, gy, dim3(256), 0, s, src + fr.in.c_off, dst + fr.out.c_off, gc, rb / 2, h->H / 2);
        } else hipLaunchKernelGGL(copy, grid, dim3(256), 0, s, src, dst, g, rb, h->H);
        HIPCHK(hipGetLastError());
    }
    return MM_OK;
}

// k_convert's quads: W % 4 == 0 and the fused compose's alignments, plus one:
// NV12 in reads a luma dword per row, so its luma rows too start on multiples of 4
static bool convert_quads_aligned(const mm_handle *h, const uint8_t *in, const uint8_t *out, const Frames &fr, int n)
{
    return h->W % 4 == 0 && k34_quads_aligned(h, in, out, fr, n) &&
           (fr.fi->kfmt != kFmtNV12 || rows_aligned(*fr.fi, in, fr.in, h->H, n, 4, 1));
}
// The passthrough frames of a convert call: the plain conversion (k_convert),
// one launch for the n frames.  The decode's coefficients over the chroma code
// scale (of the 16-bit word for P010) travel in Cvt; BT.601's are its standing
// six-digit ones (include/mm.h).
static int convert_frames(mm_handle *h, const uint8_t *in, uint8_t *out, int n, const Frames &fr, hipStream_t s)
{
    if (n <= 0) return MM_OK;
    const Geo g = geo_of(h, fr);
    Cvt cv = {0.0f, 0.0f, 0.0f, 0.0f};
    if (fr.fi->ycc()) {   // (a decode: NV12 or P010 in)
        const int fmt = fr.fmt;
        const CodeRange r = code_range(*fr.fi, fr.fi->full(fmt));
        const double cs = r.cs * r.u;
        double rcr = 1.402, gcb = -0.344136, gcr = -0.714136, bcb = 1.772;
        if (fmt_matrix(fmt)) {
            double kr, kb;
            matrix_krkb(fmt, &kr, &kb);
            const double kg = 1.0 - kr - kb;
            rcr = 2.0 * (1.0 - kr), gcb = -2.0 * kb * (1.0 - kb) / kg, gcr = -2.0 * kr * (1.0 - kr) / kg,
            bcb = 2.0 * (1.0 - kb);
        }
        cv.rcr = (float)(rcr / cs), cv.gcb = (float)(gcb / cs), cv.gcr = (float)(gcr / cs), cv.bcb = (float)(bcb / cs);
    }
    const bool quad = convert_quads_aligned(h, in, out, fr, n);
    const size_t nb = (size_t)((h->W + 3) / 4) * (size_t)(h->H / 2);
    const int per = (int)std::min<size_t>((size_t)n, std::max<size_t>(1, ((size_t)1 << 38) / nb));   // (grid x < 2^31)
    for (int f0 = 0; f0 < n; f0 += per) {
        const int m = std::min(per, n - f0);
        const dim3 grid((unsigned)((nb * m + 255) / 256));
        const uint8_t *src = in + fr.in.stride * f0;
        uint8_t *dst = out + fr.out.stride * f0;
#define MM_CONVERT_LAUNCH(F)                                                                              \
        do {                                                                                              \
            if (quad) hipLaunchKernelGGL((k_convert<F, true>), grid, dim3(256), 0, s, src, dst, g, cv, m); \
            else hipLaunchKernelGGL((k_convert<F, false>), grid, dim3(256), 0, s, src, dst, g, cv, m);    \
        } while (0)
        MM_MIXED_SWITCH(fr, MM_CONVERT_LAUNCH(FMT_))
#undef MM_CONVERT_LAUNCH
        HIPCHK(hipGetLastError());
    }
    return MM_OK;
}

// ---- MM_MODE_STEERABLE (mm_steer.hpp) -----------------------------------
static int steer_bands(const mm_handle *h)
{
    const int nmid = h->spec.L >= 3 ? h->spec.L - 2 : 0;
    return nmid * (h->spec.O / 2);
}
// state planes: phi (DIFF reads only the previous local phase), + u_h, u_l (IIR)
static int steer_planes(const mm_handle *h) { return h->spec.filt == MM_FILTER_IIR ? 3 : 1; }
static size_t steer_plane_floats(const mm_handle *h)
{
    return (size_t)steer_bands(h) * h->geo.Hn * (h->geo.Wy + 4);
}
static size_t steer_state_bytes(const mm_handle *h)
{
    return sizeof(float) * steer_planes(h) * steer_plane_floats(h);
}
// Band buffers and the temporal state planes for the current levels and
// orientations.  Reallocated (state invalid) only when those change, never
// by mm_set_batch: the per-batch spectra Fb grow separately (ensure_frames).
// frames of one k_sb_cols launch chunk (MM_SB_CF, 2 .. 16: k_sb_rows' write
// mask holds a bit per frame of its launch; N = 4096: chunks of 2, launched
// per frame)
static int sb_cols_frames(const mm_handle *h)
{
    return h->N >= 4096 ? 2 : std::min(16, std::max(2, h->sb_cf));
}
static int steer_alloc(mm_handle *h, hipStream_t s)
{
    const int nb = steer_bands(h);
    const size_t fstride = (size_t)(h->N / 2 + 1) * h->N;
    int rc = ensure_frames(h, reinterpret_cast<void **>(&h->d_Fb), &h->fb_frames, h->chunk,
                           sizeof(c2) * fstride, s);
    if (rc) return rc;
    if ((rc = ensure_yh(h, s))) return rc;
    if (h->steer_nb == nb && h->steer_planes >= steer_planes(h)) return MM_OK;
    // in-flight work of this handle may still use the old planes
    h_retire(h, h->d_T, s, true);
    h_retire(h, h->d_sst, s, true);
    h->d_T = nullptr;
    h->d_sst = nullptr;
    h->steer_nb = -1;
    h->steer_valid = false;
    // band rows of the frames one k_sb_cols launch chunk covers (sb_cols_frames:
    // at least the k_sb_rows group, a pair)
    const int tfr = sb_cols_frames(h);
    if (h_alloc(h, &h->d_T, sizeof(c2) * tfr * (size_t)(nb + 1) * h->N * t_rows(h->geo.Hn)) != hipSuccess ||
        h_alloc(h, &h->d_sst, steer_state_bytes(h) + sizeof(float)) != hipSuccess)
        return MM_ERR_OOM;
    h->steer_nb = nb;
    h->steer_planes = steer_planes(h);
    return MM_OK;
}

// Batch frames [0, n) with K1's row spectra in G: k_cols_fwd -> per frame
// k_sb_cols, k_sb_rows (the temporal filter runs frame by frame) -> K4.
// `sst`: state planes (nullptr: the handle's own, whose first frame passes
// through and seeds them when they hold no valid state; a caller's buffer
// (mm_compute_state) is always seeded).  write == false: outputs pass through,
// the state keeps following the input.
template <int LOG2N>
static int run_steer(mm_handle *h, const uint8_t *in, uint8_t *out, int n, const Frames &fr, float *sst,
                     bool write, hipStream_t s, const c2 *G)
{
    constexpr int N = 1 << LOG2N;
    int rc;
    if ((rc = steer_alloc(h, s))) return rc;   // may invalidate the handle's planes
    const int seed = sst ? 1 : (h->steer_valid ? 0 : 1);
    if (!sst) sst = h->d_sst;
    const size_t fstride = (size_t)(N / 2 + 1) * N;
    const int gpw = groups_per_wg<LOG2N>();
    const size_t lds = lds_fft_bytes<LOG2N>();
    {
        const int total = n * (N / 2 + 1);
        ProfScope ps(h, s, MM_K_COLS, n);
        hipLaunchKernelGGL((k_cols_fwd<LOG2N>), dim3((total + gpw - 1) / gpw),
                           dim3(wg_threads<LOG2N>()), lds, s, G, h->g_stride, h->d_Fb,
                           fstride, total, h->geo, h->d_tw);
        HIPCHK(hipGetLastError());
    }
    const size_t band_stride = (size_t)N * t_rows(h->geo.Hn);
    // DIFF reads and writes only the phi plane (a caller's DIFF state buffer
    // holds just that plane); IIR the three
    const size_t plane = steer_planes(h) == 3 ? steer_plane_floats(h) : 0;
    // frames in pairs: both frames' band columns, then one k_sb_rows launch
    // whose workgroups carry the first frame's new state to the second in
    // registers (MM_SB_NF=1: one frame per launch)
    const size_t t_stride = band_stride * (size_t)(steer_bands(h) + 1);
    // frames of a k_sb_rows group: 2 or 1 (fours: C3 k_sb_rows -1.3 % but
    // k_sb_cols +2.3 %, 1080p k_sb_rows +16 % at 4 waves per SIMD,
    // profiles/r06h_sb_rows_layout_ab.txt)
    const int nfm = h->sb_nf >= 2 ? 2 : 1;
    // k_sb_cols runs the band columns of sb_cf (MM_SB_CF, default 8) frames per
    // launch at N <= 2048 (blockIdx.y: frame), then the chunk's k_sb_rows
    // groups: the kernel boundaries are what it saves (1080p O = 8 DIFF, same
    // call: 1 / 2 / 4 / 8 frames per launch 5.33k / 5.54k / 5.64k / 5.67k
    // frames/s; 1.85 GB of band rows at 8); per frame at N = 4096, whose
    // 2,048-workgroup launches gain nothing from it (C3 k_sb_cols 424 -> 430
    // us at 2; profiles/r06h_sb_rows_layout_ab.txt)
    const int cf = sb_cols_frames(h);   // >= nfm
    for (int c0 = 0; c0 < n; c0 += cf) {
        const int cn = std::min(cf, n - c0);
        {
            ProfScope ps(h, s, MM_K_COLS, 0);
            const int g2 = sb_groups<LOG2N>();
            // the staging [Hn][GPW] gets its own LDS area where it costs no
            // residency: two workgroups per CU, 80 KB each (1080p: 18.4 +
            // 8.8 KB, 2160p: 36.9 + 17.5 KB); else it aliases the exchange
            // buffers (one more barrier per band, and a band's stores cannot
            // overlap the next band's transform)
            const size_t lx = sizeof(c2) * (size_t)g2 * lds_complex<N>(),
                         ls = sizeof(c2) * (size_t)g2 * sb_stg_stride(h->geo.Hn, N);   // (whole row groups)
            const int own = lx + ls <= 81920 ? 1 : 0;
            const int per = LOG2N >= 12 ? 1 : cn;
            for (int f = 0; f < cn; f += per) {
                hipLaunchKernelGGL((k_sb_cols<LOG2N>), dim3((N + g2 - 1) / g2, per), dim3(sb_threads<LOG2N>()),
                                   lx + (own ? ls : 0), s, h->d_Fb + fstride * (c0 + f), h->d_T + t_stride * f,
                                   band_stride, h->geo, h->spec, h->d_tw, own, fstride, t_stride);
                HIPCHK(hipGetLastError());
            }
        }
        for (int k = c0; k < c0 + cn;) {
            const int left = c0 + cn - k;
            const int nf = left >= nfm ? nfm : 1;
            // the chunk's whole groups of nf frames in one launch, each
            // workgroup running them one after the other (IIR: a launch per group)
            const int ng = h->spec.filt != MM_FILTER_IIR ? left / nf : 1;
            const int reset = k < seed;
            // bit f: frame k + f's Yh (the stream's first frame passes through)
            const int wmask = write ? (((1 << (ng * nf)) - 1) & ~(reset ? 1 : 0)) : 0;
            ProfScope ps(h, s, MM_K_ROWS_INV, __builtin_popcount(wmask));
            constexpr int rg = sb_rows_groups<LOG2N>();
            const dim3 grid((h->geo.Hn + rg - 1) / rg), block(sb_rows_threads<LOG2N>());
            const size_t rlds = sizeof(c2) * (size_t)rg * lds_complex<N>();
            float *yh = h->d_Yh + h->yh_stride * k;
            c2 *tk = h->d_T + t_stride * (k - c0);
#define MM_SB_ROWS(IIRV, NFV)                                                                              \
            hipLaunchKernelGGL((k_sb_rows<LOG2N, IIRV, NFV>), grid, block, rlds, s, tk, band_stride, t_stride, \
                               yh, h->yh_stride, sst, sst + plane, sst + 2 * plane, reset, wmask, h->geo,   \
                               h->spec, h->blur, h->d_tw, ng)
            if (h->spec.filt == MM_FILTER_IIR) {
                if (nf == 2) MM_SB_ROWS(true, 2);
                else MM_SB_ROWS(true, 1);
            } else {
                if (nf == 2) MM_SB_ROWS(false, 2);
                else MM_SB_ROWS(false, 1);
            }
#undef MM_SB_ROWS
            HIPCHK(hipGetLastError());
            k += ng * nf;
        }
    }
    if (sst == h->d_sst) h->steer_valid = true;
    if (!write) return out ? copy_frames(h, in, out, n, fr, s) : MM_OK;
    if (seed && (rc = copy_frames(h, in, out, 1, fr, s))) return rc;
    return launch_k4(h, in, out, seed, n, fr, s);
}

// ProcessDebugView (.cs:119-123, :234-257) for batch frames [first, n) whose
// row spectra are in G: k_dbg_cols (view textures) -> k_dbg_out (crop or split
// screen).  The state follows the input (.cs:122): the caller's slot update.
template <int LOG2N>
static int run_debug(mm_handle *h, uint8_t *out, int n, int first, const Frames &fr, hipStream_t s,
                     const c2 *G)
{
    constexpr int N = 1 << LOG2N;
    if (n <= first) return MM_OK;
    const size_t tex_stride = (size_t)2 * N * N;
    // lazily (only handles that show a debug view pay for it), sized for the batch
    int rc = ensure_frames(h, reinterpret_cast<void **>(&h->d_dbg), &h->dbg_frames, h->chunk,
                           sizeof(float) * tex_stride, s);
    if (rc) return rc;
    if (!h->d_tw_half) {
        std::vector<c2> twh(N / 2);
        for (int k = 0; k < N / 2; ++k) {
            const double a = -2.0 * M_PI * (double)k / (double)(N / 2);
            twh[k] = mk((float)cos(a), (float)sin(a));
        }
        HIPCHK(h_alloc(h, &h->d_tw_half, sizeof(c2) * (N / 2)));
        HIPCHK(hipMemcpyAsync(h->d_tw_half, twh.data(), sizeof(c2) * (N / 2), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    const int m = n - first;
    constexpr int T = fft_T<LOG2N - 1>();
    hipLaunchKernelGGL((k_dbg_cols<LOG2N>), dim3(m * N), dim3(2 * T),
                       2 * sizeof(c2) * lds_complex<N / 2>(), s, G, h->g_stride, h->d_dbg,
                       tex_stride, first, h->p.show_magnitude, h->p.show_phase, h->geo,
                       h->d_tw_half);
    HIPCHK(hipGetLastError());
    const size_t tot = (size_t)m * h->W * h->H;
    const dim3 grid((unsigned)((tot + 255) / 256));
    MM_FMT_SWITCH_FULLRES(fr.fi, hipLaunchKernelGGL((k_dbg_out<FMT_>), grid, dim3(256), 0, s, h->d_dbg, tex_stride,
                                          out, first, m, h->p.show_magnitude, h->p.show_phase, geo_of(h, fr)))
    HIPCHK(hipGetLastError());
    return MM_OK;
}

// One batch of `n` consecutive frames (n <= chunk), all on the device.
template <int LOG2N>
static int run_chunk(mm_handle *h, const uint8_t *in, uint8_t *out, int n, const Frames &fr,
                     hipStream_t s)
{
    const bool mag = h->p.apply_magnification != 0;
    const bool dbg = h->p.show_magnitude || h->p.show_phase;
    // the steerable path's state is its local-phase planes; every other path
    // needs G_{t-1} in the G slot (a steerable mm_set_state leaves it unset:
    // the next pyramid frame then passes through, as after a reset)
    const bool steer = !dbg && h->p.mode == MM_MODE_STEERABLE;
    const bool have = h->has_state && (steer || h->g_valid);
    const int first = have ? 0 : 1;
    // Held reference (mm_set_hold; pyramid and standard mode only: the entry
    // points refuse the rest): the batch pairs with the state slot and leaves
    // it where it is; without state, frame 0 becomes the reference.
    const bool hold = h->hold;
    int rc, base;
    if (first && (rc = copy_frames(h, in, out, 1, fr, s))) return rc;
    if (hold && !mag && have) return copy_frames(h, in, out, n, fr, s);   // nothing else happens: no K1
    if ((rc = place_batch(h, n, s, &base))) return rc;
    c2 *G = h->d_G + h->g_stride * base;
    // G_{t-1}: the state slot; a stream's first frame primes with itself (its
    // Q is computed and not used: it passes through)
    const c2 *Gprev = have ? h->d_G + h->g_stride * h->gs : G;
    if (!dbg && h->p.mode != MM_MODE_STEERABLE && !mag) {
        // applyMotionMagnification == false: Blit(source, destination) (.cs:139),
        // but previousSourceTexture still follows the input (.cs:142): K1 of
        // the batch's last frame only.
        const int from = first ? 1 : 0;
        if (n > from &&
            (rc = copy_frames(h, in + fr.in.stride * from, out + fr.out.stride * from, n - from, fr, s)))
            return rc;
        // (hold, no state yet: the call's first frame is the reference)
        if ((rc = launch_k1<LOG2N>(h, in + fr.in.stride * (hold ? 0 : n - 1), 1, fr, s, G))) return rc;
        h->gs = base;
        h->has_state = h->g_valid = true;
        return MM_OK;
    }
    if ((rc = launch_k1<LOG2N>(h, in, n, fr, s, G))) return rc;
    if (dbg) {
        h->steer_valid = false;   // the debug path does not advance the local-phase state
        rc = run_debug<LOG2N>(h, out, n, first, fr, s, G);
    } else if (h->p.mode == MM_MODE_STEERABLE) {
        if (first) h->steer_valid = false;
        // two transforms per band workgroup: N <= 4096 (mm_create refuses more)
        if constexpr (LOG2N <= 12) rc = run_steer<LOG2N>(h, in, out, n, fr, nullptr, mag, s, G);
        else rc = MM_ERR_UNSUPPORTED;
    } else {
        if ((rc = launch_k2<LOG2N>(h, n, Gprev, G, s, hold))) return rc;
        rc = launch_k3<LOG2N>(h, h->d_Q, in, out, first, n, fr, s);
    }
    if (rc) return rc;
    if (hold && have) return MM_OK;   // gs stays: the batch's slots are clear of it (place_batch)
    h->gs = hold ? base : base + n - 1;   // the state follows the input in every mode (.cs:142)
    h->has_state = h->g_valid = true;
    return MM_OK;
}

template <int LOG2N>
static int run_stream(mm_handle *h, const uint8_t *in, uint8_t *out, int count, const Frames &fr,
                      hipStream_t s)
{
    for (int f0 = 0; f0 < count; f0 += h->chunk) {
        const int n = std::min(h->chunk, count - f0);
        int rc = run_chunk<LOG2N>(h, in + fr.in.stride * f0, out + fr.out.stride * f0, n, fr, s);
        if (rc) return rc;
    }
    return MM_OK;
}

// The state frame `in` leaves behind: its row spectra (K1) straight into dst;
// steerable DIFF: its local phases (K1 to a free G slot, then the band path).
template <int LOG2N>
static int compute_state(mm_handle *h, const uint8_t *in, const Frames &fr, void *dst, hipStream_t s)
{
    int rc;
    if (h->p.mode == MM_MODE_STEERABLE) {
        int base;
        if ((rc = place_batch(h, 1, s, &base))) return rc;
        c2 *G = h->d_G + h->g_stride * base;
        if ((rc = launch_k1<LOG2N>(h, in, 1, fr, s, G))) return rc;
        if constexpr (LOG2N <= 12)
            return run_steer<LOG2N>(h, in, nullptr, 1, fr, reinterpret_cast<float *>(dst), false, s, G);
        else
            return MM_ERR_UNSUPPORTED;
    }
    return launch_k1<LOG2N>(h, in, 1, fr, s, reinterpret_cast<c2 *>(dst));
}

// One frame of each lane of `mask` (mm_process_lanes_mask; mm_process_lanes
// is the mask of all lanes): frame k of the buffers is lane k's next frame.  K1
// of a selected lane writes the slot of the bank that does not hold its state
// (a lane without state: its neighbour's bank, so that it joins a run), one
// launch per run of consecutive selected lanes that write one bank; one K2 over
// the selected lanes (launch_k2_lanes: k_cols_lanes_sel finds each lane's two
// slots by its bank bit); then K3 + K4 from the lanes' Q.  A lane without
// state passes through (its K2 result is computed and not used, as a stream's
// first frame's is): the compose runs over the runs of selected lanes that
// have state, one launch when all have, so a passthrough frame is never
// composed over first (in == out).  The selected lanes' bank bits flip: no
// state copy, and a lane that sits the call out keeps its slot, its bit and
// its flag.
template <int LOG2N>
static int run_lanes(mm_handle *h, uint64_t mask, const uint8_t *in, uint8_t *out, const Frames &fr, hipStream_t s)
{
    if constexpr (LOG2N > 12) return MM_ERR_UNSUPPORTED;   // (mm_set_lanes refuses N = 8192)
    else {
        const int n = h->lanes;
        const auto bit = [](uint64_t m, int k) { return (int)((m >> k) & 1); };
        // wr: the bank each selected lane's K1 writes
        uint64_t wr = ~h->lane_bank & h->lane_state & mask;
        for (int k = 0; k < n; ++k) {
            if (!bit(mask, k) || bit(h->lane_state, k)) continue;
            int w;
            if (k > 0 && bit(mask, k - 1)) w = bit(wr, k - 1);
            else {
                int j = k + 1;
                while (j < n && bit(mask, j) && !bit(h->lane_state, j)) ++j;
                w = j < n && bit(mask, j) ? bit(wr, j) : 1 - bit(h->lane_bank, k);
            }
            wr |= (uint64_t)w << k;
        }
        const size_t bank = h->g_stride * (size_t)n;
        const bool mag = h->p.apply_magnification != 0;
        int rc;
        // In place (in == out; decided for any overlap of the two buffers'
        // selected frames): the compose reads source rows next to the ones it
        // writes, of other workgroups' strips too, so the frames it composes
        // are copied aside first, tight, and composed from there.  Their
        // buffer is made before anything is queued: a failed allocation
        // leaves the handle and every lane as they were.
        bool aside = false;
        mm_surface t;
        (void)surf_tight(h->W, h->H, fr.fmt, &t);
        if (mag && (mask & h->lane_state)) {
            const int lo = __builtin_ctzll(mask), hi = 64 - __builtin_clzll(mask);
            const uint8_t *i0 = in + fr.in.stride * lo, *i1 = in + fr.in.stride * hi;
            const uint8_t *o0 = out + fr.out.stride * lo, *o1 = out + fr.out.stride * hi;
            aside = i0 < o1 && o0 < i1;
            const size_t need = t.frame_stride * (size_t)n;
            if (aside && h->lsrc_bytes < need) {
                uint8_t *p = nullptr;
                if (h_alloc(h, &p, need) != hipSuccess) return MM_ERR_OOM;
                h_retire(h, h->d_Lsrc, s, true);
                h->d_Lsrc = p;
                h->lsrc_bytes = need;
            }
        }
        // (magnification off: a held lane that has state is copied through and
        // nothing else happens to it: no K1)
        const uint64_t k1 = mag ? mask : mask & ~(h->lane_hold & h->lane_state);
        for (int a = 0, b; a < n; a = b) {
            b = a + 1;
            if (!bit(k1, a)) continue;
            while (b < n && bit(k1, b) && bit(wr, b) == bit(wr, a)) ++b;
            c2 *G = h->d_LG + bank * bit(wr, a) + h->g_stride * a;
            if ((rc = launch_k1<LOG2N>(h, in + fr.in.stride * a, b - a, fr, s, G))) return rc;
        }
        // (off: Blit(source, destination) (.cs:139); every selected lane's state follows its input)
        if (mag && (rc = launch_k2_lanes<LOG2N>(h, mask, ~wr & mask, s))) return rc;
        // (K1 has read the frames by now; a passthrough onto itself is nothing)
        const uint8_t *src = in;
        Frames fc = fr;
        if (aside) {
            Frames up = fr;   // the caller's frames -> the tight copies
            up.ofmt = fr.fmt;
            up.fo = fr.fi;
            up.out = surf_lay(t);
            up.packed = !fr.mixed() ? fr.packed : false;
            fc.in = up.out;
            fc.packed = false;
            for (int a = 0, b; a < n; a = b) {
                b = a + 1;
                if (!bit(mask & h->lane_state, a)) continue;
                while (b < n && bit(mask & h->lane_state, b)) ++b;
                if ((rc = copy_frames(h, in + fr.in.stride * a, h->d_Lsrc + t.frame_stride * a, b - a, up, s)))
                    return rc;
            }
            src = h->d_Lsrc;
        }
        for (int a = 0, b; a < n; a = b) {
            b = a + 1;
            if (!bit(mask, a)) continue;
            const bool st = mag && bit(h->lane_state, a);
            while (b < n && bit(mask, b) && (mag && bit(h->lane_state, b)) == st) ++b;
            if (st) rc = launch_k3<LOG2N>(h, h->d_LQ, src, out, a, b, fc, s);
            else rc = copy_frames(h, in + fr.in.stride * a, out + fr.out.stride * a, b - a, fr, s);
            if (rc) return rc;
        }
        // a held lane that had state keeps its bank bit: its K1 wrote the
        // other slot, K2 read both, and the next call overwrites that slot
        const uint64_t flip = mask & ~(h->lane_hold & h->lane_state);
        h->lane_bank = (h->lane_bank & ~flip) | (wr & flip);
        h->lane_state |= mask;
        return MM_OK;
    }
}

// MM_ONLY_LOG2N=n (experiment builds only): instantiate one padded size, so an
// A/B variant compiles in a fraction of the full build's time

// The per-size entry points (defined in mm_n<L>.hip by MM_SIZE_ENTRIES(L),
// or in mm_api.hip itself for a one-size experiment build, MM_ONLY_LOG2N)
#define MM_SIZE_DECLS(L)                                                                            \
    int mm_size_set_attrs_##L(mm_handle *h);                                                        \
    int mm_size_stream_##L(mm_handle *h, const uint8_t *in, uint8_t *out, int count,                \
                           const Frames &fr, hipStream_t s);                                        \
    int mm_size_compute_state_##L(mm_handle *h, const uint8_t *in, const Frames &fr, void *dst,     \
                                  hipStream_t s);                                                   \
    int mm_size_lanes_##L(mm_handle *h, uint64_t mask, const uint8_t *in, uint8_t *out, const Frames &fr, hipStream_t s);
#define MM_SIZE_ENTRIES(L) MM_SIZE_ENTRIES_(L)
#define MM_SIZE_ENTRIES_(L)                                                                         \
    int mm_size_set_attrs_##L(mm_handle *h) { return set_attrs<L>(h->W); }                          \
    int mm_size_stream_##L(mm_handle *h, const uint8_t *in, uint8_t *out, int count,                \
                           const Frames &fr, hipStream_t s)                                         \
    {                                                                                               \
        return run_stream<L>(h, in, out, count, fr, s);                                             \
    }                                                                                               \
    int mm_size_compute_state_##L(mm_handle *h, const uint8_t *in, const Frames &fr, void *dst,     \
                                  hipStream_t s)                                                    \
    {                                                                                               \
        return compute_state<L>(h, in, fr, dst, s);                                                 \
    }                                                                                               \
    int mm_size_lanes_##L(mm_handle *h, uint64_t mask, const uint8_t *in, uint8_t *out, const Frames &fr, hipStream_t s) \
    {                                                                                               \
        return run_lanes<L>(h, mask, in, out, fr, s);                                                     \
    }
MM_SIZE_DECLS(4)
MM_SIZE_DECLS(5)
MM_SIZE_DECLS(6)
MM_SIZE_DECLS(7)
MM_SIZE_DECLS(8)
MM_SIZE_DECLS(9)
MM_SIZE_DECLS(10)
MM_SIZE_DECLS(11)
MM_SIZE_DECLS(12)
MM_SIZE_DECLS(13)
