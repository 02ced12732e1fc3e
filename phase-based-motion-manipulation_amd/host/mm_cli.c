/*
 * mm_cli.c — C host driver over the C-ABI (include/mm.h).
 *
 * Plays the role of the Unity camera that calls OnRenderImage once per frame
 * (Assets/Scripts/MotionMagnificationProcessor.cs:101): it generates a
 * synthetic RGBA8 stream on the device, or reads a clip, runs
 * the magnifier over it and reports throughput.
 *
 *   mm_cli [-w W] [-h H] [-n frames] [-l levels] [-s phase_scale]
 *          [-b frames_per_call] [-i in.{rgba,y4m}] [-o out.{rgba,y4m}] [-d device]
 *          [--full-range] [--srgb] [--nv12] [--p010] [--matrix 601|709|2020] [--mono]
 *          [--yuy2] [--uyvy] [--y210] [--v210] [--ppm [--bgr | --bgra]] [--i420] [--i010] [--out-rgba8 | --out-bgra8] [--out-nv12]
 *          [--standard] [--show-magnitude] [--show-phase]
 *          [--orientations O] [--iir] [--halo K] [--surface-align P,R] [--lanes M]
 *          [--hold R]
 *          [--checksum] [--ring-world G --ring-rank R --ring-id FILE]
 *          [--ring-local G [--compare]]
 *
 * --orientations O (4/6/8): MM_MODE_STEERABLE extension,
 * DIFF temporal filter, or IIR with --iir.  A sharded IIR stream warms each
 * rank's filter on the halo of frames before its chunk (mm_ring_step_halo;
 * --halo K overrides mm_ring_halo_frames()).  --compare (with --ring-local):
 * the single-handle stream afterwards, frame by frame against the ring's
 * outputs ("cmp t maxabs ndiff" lines and a summary).
 *
 * --ring-*: frame-sharded synthetic stream over an RCCL ring (include/mm_ring.h,
 * SURVEY.md §8e), one process per GPU: rank R of G processes chunks of -b
 * frames, the ring carries the chunk-boundary state; rank 0 writes the ring id
 * to FILE, the others read it.  --checksum prints "frame <t> <byte sum>" per
 * output frame (global frame index t), so a sharded run can be compared with
 * the single-process stream.
 *
 * --ring-local G: the same frame-sharded stream at world G inside ONE process
 * on one device, one thread (and one mm_handle) per rank, through the ring's
 * test-only local transport (host/mm_ring_local.h): the product's mm_ring_step
 * logic at world > 1 on a one-GPU box.  Checksums are printed in global frame
 * order after every rank has finished.
 *
 * .y4m input: 8-bit 4:2:0 / 4:4:4 / mono YUV4MPEG2, geometry from its header
 * (host/y4m.h, BT.601 limited range unless --full-range); .y4m output is 4:4:4
 * at the input's frame rate.  Any other extension is raw RGBA8 (-w/-h).
 * --srgb: the 8-bit frames are sRGB-encoded (video and display-referred
 * clips are), processed in linear light as Unity's Linear colour space does
 * (MM_RGBA8_SRGB: decoded on read, encoded on write); default UNORM.
 * The input-format options (--nv12 --p010 --i420 --i010 --mono --yuy2 --uyvy
 * --y210 --v210 --ppm; k_in_opts below has a row each): at most one, and none goes
 * with --srgb, the ring modes, --out-nv12 or, but for --mono, the debug views;
 * --out-rgba8 goes with --nv12 and --p010 alone; --matrix and --full-range go
 * with the Y'CbCr ones (all but --mono and --ppm), which need even sizes.
 * Each names the one input it takes; every refusal is a usage error (status
 * 2) before the output file is created and before the device is touched.
 * --nv12: a 4:2:0 .y4m input goes to the device as it is stored, as MM_NV12
 * frames (MM_NV12_FULL with --full-range): the chroma planes are interleaved
 * on the way in and split on the way out (a C420 .y4m; any other extension:
 * the raw NV12 frames), and no colour arithmetic runs on the host.
 * --p010: the same for a 10-bit 4:2:0 .y4m input (C420p10), sent as MM_P010
 * frames (MM_P010_FULL with --full-range): the chroma planes are interleaved
 * and every sample shifted left by 6 on the way in, the reverse on the way out
 * (a C420p10 .y4m; any other extension: the raw P010 frames).  Bit depths are never
 * converted silently: an 8-bit input with --p010 and a 10-bit input without it
 * are refused.
 * --matrix 601|709|2020 (default 601): the Y'CbCr matrix of an --nv12,
 * --p010, --yuy2, --uyvy, --y210 or --v210 clip (HD content is BT.709, UHD BT.709 or BT.2020), OR-ed onto the
 * frame format as MM_MATRIX_BT709 / MM_MATRIX_BT2020.  A .y4m header has no
 * matrix tag, so files are the same whatever the value.  Only with --nv12,
 * --p010, --yuy2, --uyvy, --y210 or --v210: the host's own RGBA conversion of a .y4m is BT.601.
 * --mono: a mono .y4m input (Cmono, Cmono10, Cmono12, Cmono16: a grayscale
 * camera's or ffmpeg's gray / gray10le / gray12le / gray16le frames) goes to
 * the device as it is stored, as MM_Y8 / MM_Y10 / MM_Y12 / MM_Y16 frames by the
 * header's depth: one sample per pixel each way, no conversion, odd sizes, the
 * standard and steerable modes and the debug views included.  The output is a
 * .y4m of the same Cmono* type (any other extension: the raw frames).  There
 * is no matrix and no range: not with --matrix or --full-range.
 * Without --mono a Cmono input is expanded to RGBA8 on the host, as before.
 * --yuy2 / --uyvy: an 8-bit 4:2:2 .y4m input (C422: a capture device's frames,
 * ffmpeg's yuv422p) goes to the device as packed macropixels, Y0 Cb Y1 Cr as
 * MM_YUY2 or Cb Y0 Cr Y1 as MM_UYVY (_FULL with --full-range, a matrix bit
 * with --matrix): the planes are interleaved on the way in and split on the
 * way out (a C422 .y4m, the same file for both flags; any other extension: the
 * raw packed frames), and no colour arithmetic runs on the host.
 * A C422 input needs one of the two
 * flags: the host has no 4:2:2 to RGBA conversion.
 * --y210: a 10-bit 4:2:2 .y4m input (C422p10: planar, the code in the low 10
 * bits of each word; ffmpeg's yuv422p10le) goes to the device as MM_Y210
 * frames, words Y0 Cb Y1 Cr with the code << 6 (_FULL with --full-range, a
 * matrix bit with --matrix): the planes are interleaved and shifted on the way
 * in and split on the way out (a C422p10 .y4m; any other extension: the raw
 * Y210 frames), and no colour arithmetic runs on the host.
 * A C422p10 input needs --y210 or --v210: it is
 * never converted on the host.
 * --v210: the same C422p10 .y4m input goes to the device as MM_V210 frames,
 * the capture cards' layout of three 10-bit codes per dword (include/mm.h),
 * rows at the standard pitch 128 ceil(W / 48): the container has no v210 tag,
 * so each frame is packed on the host on the way in and unpacked on the way
 * out (host/v210.h; shifts only, no colour arithmetic; a C422p10 .y4m; any
 * other extension: the raw v210 frames).  The output file is --y210's, byte for
 * byte.  --matrix, --full-range, --surface-align (P a multiple of 16) and
 * --checksum as usual; --y210's usage errors.
 * --ppm: the input (-i) is a stream of concatenated binary PPM images (P6,
 * maxval 255, one size: what ffmpeg -f image2pipe -vcodec ppm writes; host/ppm.h).
 * Its frames go to the device as MM_RGB24 as they lie, 3 bytes per pixel each
 * way, and -o gets the same container back.  --bgra widens every image on the
 * host to B G R 255 and processes it as MM_BGRA8, the alpha dropped on write:
 * the output file is --ppm's byte for byte (it shows the BGRA path; not with
 * --bgr).  --bgr swaps R and B on read and
 * on write and sends MM_BGR24 (the files are the run without it, byte for
 * byte).  Every size, -l, -s, -b, --standard and --surface-align as usual.
 * Not with --matrix, --full-range or a .y4m on either side.
 * --i420: an 8-bit 4:2:0 .y4m input (C420) goes to the device as its frames lie
 * in the file, as MM_I420 frames (MM_I420_FULL with --full-range, a matrix bit
 * with --matrix): three planes, no interleave on the way in and no split on the
 * way out (a C420 .y4m; any other extension on either side: the raw I420
 * frames, -w/-h).  The output file is --nv12's, byte for byte.  -l, -s, -b,
 * --standard, --surface-align and --checksum as usual.
 * --i010: a 10-bit 4:2:0 .y4m input (C420p10) goes to the device as its frames
 * lie in the file, as MM_I010 frames (MM_I010_FULL with --full-range, a matrix
 * bit with --matrix): three planes of words with the code in the low 10 bits,
 * no interleave and no shift on the way in, no split on the way out (a C420p10
 * .y4m; any other extension on either side: the raw I010 frames, -w/-h).  The
 * output file is --p010's, byte for byte.  -l, -s, -b, --standard,
 * --surface-align and --checksum as usual.
 * --surface-align P,R: the device frames, input and output, are held in
 * mm_surface_aligned(W, H, format, P, R) surfaces (256,16: a hardware
 * decoder's layout) and go through mm_process_stream_surfaces; for every input
 * format, --nv12, --p010, --yuy2, --uyvy and --y210 included.  Files and checksums are those of the
 * run without the flag, byte for byte.  Not with the ring modes.
 * --out-bgra8 (with --nv12 or --p010): --out-rgba8 with MM_BGRA8 as the output
 * format, raw frames only: --out-rgba8's output with bytes 0 and 2 of every
 * pixel exchanged.
 * --out-rgba8 (with --nv12 or --p010): decode on the way out.  The frames go
 * in as stored and raw MM_RGBA8 frames come out, through
 * mm_process_stream_convert: -o gets the raw RGBA8 frames, or, a .y4m, the 4:4:4
 * file the default RGBA8 path writes from them.  Refused without --nv12 /
 * --p010 and with --out-nv12.
 * --out-nv12 (with the RGBA8 input path: a synthetic stream, raw RGBA8 frames,
 * or a .y4m the host expands as above): encode on the way out.  MM_RGBA8 frames
 * go in and NV12 frames come out: -o gets a C420 .y4m, or the raw NV12 frames.
 * --full-range and --matrix then name the OUTPUT code (MM_NV12_FULL, a matrix
 * bit) and nothing else: a .y4m input is expanded as BT.601 limited range.
 * Refused with --out-rgba8, every input-format option, --srgb, the debug
 * views, the ring modes and odd sizes.
 * With either, --surface-align lays out each side in its own format's
 * surface, and --checksum hashes the output frames, as usual.
 * --lanes M (1 .. MM_LANES_MAX): the input is M live streams interleaved, input
 * frame k being stream (lane) k % M's frame k / M, as a rig of M cameras
 * delivers them tick by tick.  One mm_process_lanes call per M frames (-b is
 * ignored); the output has the input's order.  Every format option and
 * --surface-align as usual.  The frame count (-n for a synthetic stream, else
 * the frames the input holds, -n at most) must be a multiple of M: else status
 * 2, before the output file is created.  Refused with --orientations / --iir,
 * the debug views and the ring modes.
 * --lane-drop L:T[,L:T...] (with --lanes and an input file): lane L's frame of
 * tick T, input frame T * M + L, is a frame that never arrived.  It is not
 * uploaded, and that tick's call (mm_process_lanes_mask) leaves bit L clear:
 * the lane sits the tick out and continues from the frame before.  The output
 * keeps whole ticks; a dropped slot holds the passthrough of its input frame (a
 * host copy).  Status 2, before the output file is created, without --lanes,
 * for a lane >= M, for a malformed list, and without -i or with --checksum,
 * --out-rgba8 or --out-nv12 (the host copy is no conversion).
 * --hold R: a held reference frame (mm_set_hold).  R = 0: the clip's first
 * frame is the reference throughout.  R > 0: a new reference every R frames;
 * the stream calls are split there and frames R, 2 R, ... run alone with hold
 * off (each still pairs with the old reference and becomes the new one).  Every
 * format option, --surface-align and --lanes as usual; with --lanes every lane
 * holds and R counts ticks.  Refused (status 2) with --orientations / --iir,
 * the debug views and the ring modes.
 */
#include <hip/hip_runtime_api.h>
#include <ctype.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mm.h"
#include "mm_ring.h"
#include "mm_ring_local.h"
#include "ppm.h"
#include "v210.h"
#include "y4m.h"

#include <pthread.h>
#include <stdint.h>

#include <time.h>
#include <unistd.h>

/* frame format of every 8-bit frame this driver moves (--srgb) */
static int g_fmt = MM_RGBA8;

#define CHECK(x)                                                                      \
    do {                                                                              \
        int rc_ = (x);                                                                \
        if (rc_ != MM_OK) {                                                           \
            fprintf(stderr, "%s failed: %s (%d)\n", #x, mm_strerror(rc_), rc_);       \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

static int ends_with(const char *s, const char *suf)
{
    const size_t n = strlen(s), m = strlen(suf);
    return n >= m && strcmp(s + n - m, suf) == 0;
}

/* 64-bit FNV-1a over the frame's 8-byte words (any changed byte, and any
 * moved word, changes it; a byte sum would miss permutations) */
static uint64_t frame_hash(const unsigned char *p, size_t fb)
{
    uint64_t h = 0xcbf29ce484222325ull;
    size_t i = 0;
    for (; i + 8 <= fb; i += 8) {
        uint64_t w;
        memcpy(&w, p + i, 8);
        h = (h ^ w) * 0x100000001b3ull;
    }
    for (; i < fb; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

/* hashes of n device frames, one frame copied to the host at a time */
static int hash_frames(const unsigned char *dev, size_t fb, int n, uint64_t *out)
{
    unsigned char *h = (unsigned char *)malloc(fb);
    if (!h) return 1;
    for (int k = 0; k < n; ++k) {
        if (hipMemcpy(h, dev + fb * (size_t)k, fb, hipMemcpyDeviceToHost) != hipSuccess) {
            free(h);
            return 1;
        }
        out[k] = frame_hash(h, fb);
    }
    free(h);
    return 0;
}

static void print_checksums(const unsigned char *dev, size_t fb, int n, int t0)
{
    uint64_t *hs = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)(n > 0 ? n : 1));
    if (hs && !hash_frames(dev, fb, n, hs))
        for (int k = 0; k < n; ++k) printf("frame %d %llu\n", t0 + k, (unsigned long long)hs[k]);
    free(hs);
}

/* n frames between two layouts, the W x H samples only (2D copies per plane) */
static int surf_copy(void *dst, const mm_surface *dl, const void *src, const mm_surface *sl, int W, int H, int n,
                     hipMemcpyKind kind, hipStream_t s)
{
    mm_surface t;
    if (mm_surface_tight(W, H, dl->format, &t)) return 1;
    /* sample bytes of a row (v210: the used dwords, short of the tight pitch) */
    const size_t rb = (dl->format & MM_PACK_V210) ? v210_row_bytes(W) : t.pitch;
    if (dl->pitch == t.pitch && sl->pitch == t.pitch && dl->chroma_offset == t.chroma_offset &&
        sl->chroma_offset == t.chroma_offset && dl->chroma_pitch == t.chroma_pitch &&
        sl->chroma_pitch == t.chroma_pitch && dl->frame_stride == t.frame_stride &&
        sl->frame_stride == t.frame_stride)   /* tight on both sides: one copy */
        return hipMemcpyAsync(dst, src, t.frame_stride * (size_t)n, kind, s) != hipSuccess;
    /* plane q of a frame: the luma (or only) plane, then the chroma plane or
     * planes, H / 2 rows of the tight layout's chroma row; three planes: the Cr
     * plane lies chroma_pitch x H/2 after the Cb plane */
    const int np = !t.chroma_pitch ? 1 : (dl->format & MM_PLANAR) ? 3 : 2;
    const size_t hc = (size_t)H / 2;
    for (int k = 0; k < n; ++k) {
        unsigned char *d = (unsigned char *)dst + dl->frame_stride * (size_t)k;
        const unsigned char *a = (const unsigned char *)src + sl->frame_stride * (size_t)k;
        for (int q = 0; q < np; ++q) {
            const size_t doff = q ? dl->chroma_offset + (size_t)(q - 1) * dl->chroma_pitch * hc : 0;
            const size_t soff = q ? sl->chroma_offset + (size_t)(q - 1) * sl->chroma_pitch * hc : 0;
            if (hipMemcpy2DAsync(d + doff, q ? dl->chroma_pitch : dl->pitch, a + soff, q ? sl->chroma_pitch : sl->pitch,
                                 q ? t.chroma_pitch : rb, q ? hc : (size_t)H, kind, s) != hipSuccess)
                return 1;
        }
    }
    return 0;
}

/* --lane-drop: the (lane, tick) slots of frames that never arrived */
typedef struct { int lane, tick; } lane_drop;

/* "L:T[,L:T...]", L in 0 .. M-1, T >= 0; NULL (and *n = -1) for anything else */
static lane_drop *parse_lane_drops(const char *arg, int M, int *n)
{
    size_t cap = 1;
    for (const char *c = arg; *c; ++c) cap += *c == ',';
    lane_drop *d = (lane_drop *)malloc(sizeof *d * cap);
    *n = 0;
    for (const char *c = arg; d;) {
        char *e;
        if (*c < '0' || *c > '9') break;
        const long l = strtol(c, &e, 10);
        if (*e != ':' || e[1] < '0' || e[1] > '9' || l >= M) break;
        const long t = strtol(e + 1, &e, 10);
        if (t > 0x3fffffff) break;
        d[*n].lane = (int)l;
        d[(*n)++].tick = (int)t;
        if (!*e) return d;
        if (*e != ',') break;
        c = e + 1;
    }
    free(d);
    *n = -1;
    return NULL;
}

/* the lanes of tick `tick` that take a frame */
static uint64_t tick_mask(const lane_drop *d, int nd, int M, int tick)
{
    uint64_t m = M >= 64 ? ~0ull : (1ull << M) - 1;
    for (int k = 0; k < nd; ++k)
        if (d[k].tick == tick) m &= ~(1ull << d[k].lane);
    return m;
}

/* surf_copy of the frames of `mask` among n (all of them: one copy, as ever) */
static int surf_copy_mask(void *dst, const mm_surface *dl, const void *src, const mm_surface *sl, int W, int H, int n,
                          uint64_t mask, hipMemcpyKind kind, hipStream_t s)
{
    for (int a = 0, b; a < n; a = b) {
        b = a + 1;
        if (!((mask >> (a & 63)) & 1)) continue;
        while (b < n && ((mask >> (b & 63)) & 1)) ++b;
        if (surf_copy((unsigned char *)dst + dl->frame_stride * (size_t)a, dl,
                      (const unsigned char *)src + sl->frame_stride * (size_t)a, sl, W, H, b - a, kind, s))
            return 1;
    }
    return 0;
}

/* Ring id out of band: rank 0 writes FILE (atomically), the others wait for it. */
static int ring_id(int rank, const char *path, unsigned char id[MM_RING_ID_BYTES])
{
    if (rank == 0) {
        if (mm_ring_get_id(id)) return 1;
        char tmp[4096];
        snprintf(tmp, sizeof tmp, "%s.tmp", path);
        FILE *f = fopen(tmp, "wb");
        if (!f || fwrite(id, 1, MM_RING_ID_BYTES, f) != MM_RING_ID_BYTES) return 1;
        fclose(f);
        return rename(tmp, path) != 0;
    }
    for (int tries = 0; tries < 1200; ++tries) {   /* 60 s */
        FILE *f = fopen(path, "rb");
        if (f) {
            const size_t got = fread(id, 1, MM_RING_ID_BYTES, f);
            fclose(f);
            if (got == MM_RING_ID_BYTES) return 0;
        }
        struct timespec ts = {0, 50 * 1000 * 1000};
        nanosleep(&ts, NULL);
    }
    return 1;
}

/* Frame-sharded synthetic stream: rank R of G owns frames
 * [s*G*B + R*B, s*G*B + (R+1)*B) of step s. */
static int run_ring(mm_handle *h, int W, int H, int F, int B, int dev, int world, int rank,
                    const char *id_path, int checksum, int halo)
{
    unsigned char id[MM_RING_ID_BYTES];
    if (ring_id(rank, id_path, id)) {
        fprintf(stderr, "ring id exchange through %s failed\n", id_path);
        return 1;
    }
    mm_ring *r = NULL;
    int rc = mm_ring_create(world, rank, id, dev, h, W, H, B, g_fmt, &r);
    if (rc) {
        fprintf(stderr, "mm_ring_create: %s (%s)\n", mm_strerror(rc), mm_ring_last_error());
        return 1;
    }
    const size_t fb = (size_t)W * H * 4;
    void *d_in = NULL, *d_out = NULL, *d_next = NULL, *d_halo = NULL;
    int K = 0;
    if (mm_ring_halo_frames(r, &K)) return 1;
    if (halo >= 0 && K > 0) K = halo;
    if (hipMalloc(&d_in, fb * B) != hipSuccess || hipMalloc(&d_out, fb * B) != hipSuccess ||
        hipMalloc(&d_next, fb) != hipSuccess || (K > 0 && hipMalloc(&d_halo, fb * K) != hipSuccess)) {
        fprintf(stderr, "hipMalloc failed\n");
        return 1;
    }
    hipStream_t s = (hipStream_t)mm_stream(h);
    const int steps = F / (world * B);
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    double t_proc = 0.0;
    for (int st = 0; st < steps; ++st) {
        const int t0 = st * world * B + rank * B;
        CHECK(mm_synth_frames(d_in, W, H, t0, B, 0x5EED0000ull, 0, s));
        const int last = st + 1 < steps;
        if (last) CHECK(mm_synth_frames(d_next, W, H, t0 + world * B + B - 1, 1, 0x5EED0000ull, 0, s));
        const int hk = t0 < K ? t0 : K;   /* IIR: the warm-up halo before the chunk */
        if (hk) CHECK(mm_synth_frames(d_halo, W, H, t0 - hk, hk, 0x5EED0000ull, 0, s));
        hipEventRecord(e0, s);
        rc = K > 0 ? mm_ring_step_halo(r, st, d_halo, hk, d_in, d_out, s)
                   : mm_ring_step(r, st, d_in, d_out, last ? d_next : NULL, s);
        if (rc) {
            fprintf(stderr, "mm_ring_step: %s (%s)\n", mm_strerror(rc), mm_ring_last_error());
            return 1;
        }
        hipEventRecord(e1, s);
        hipEventSynchronize(e1);
        float ms = 0.0f;
        hipEventElapsedTime(&ms, e0, e1);
        if (st > 0) t_proc += ms * 1e-3;
        if (checksum) print_checksums((const unsigned char *)d_out, fb, B, t0);
    }
    if (steps > 1 && t_proc > 0)
        printf("rank %d/%d  steps %d  frames/s per rank %.1f\n", rank, world, steps,
               (steps - 1) * B / t_proc);
    mm_ring_destroy(r);
    hipFree(d_in);
    hipFree(d_out);
    hipFree(d_next);
    hipFree(d_halo);
    return 0;
}

/* --ring-local: rank threads of one process on one device (test-only transport) */
typedef struct {
    mm_ring_hub *hub;
    const mm_params *p;
    int W, H, F, B, dev, world, rank, checksum, halo;
    uint64_t *hashes;   /* [F], global frame index */
    unsigned char *d_all;   /* --compare: every output frame, global index (device) */
    int rc;
    char err[256];
} local_rank;

static void *local_rank_main(void *arg)
{
    local_rank *a = (local_rank *)arg;
    mm_handle *h = NULL;
    mm_ring *r = NULL;
    void *d_in = NULL, *d_out = NULL, *d_next = NULL;
    const size_t fb = (size_t)a->W * a->H * 4;
    const int steps = a->F / (a->world * a->B);
    int rc;
    a->rc = 1;
    if (hipSetDevice(a->dev) != hipSuccess) { snprintf(a->err, sizeof a->err, "hipSetDevice"); return NULL; }
    if ((rc = mm_create(a->W, a->H, a->p, a->dev, &h)) || (rc = mm_set_batch(h, a->B)) ||
        (rc = mm_ring_create_local(a->hub, a->rank, a->dev, h, a->W, a->H, a->B, g_fmt, &r))) {
        snprintf(a->err, sizeof a->err, "setup: %s (%s)", mm_strerror(rc), mm_ring_last_error());
        /* a rank that cannot join would leave the others at the hub's
         * barrier: report and stop the process */
        fprintf(stderr, "rank %d: %s\n", a->rank, a->err);
        exit(1);
    }
    int K = 0;
    void *d_halo = NULL;
    if (mm_ring_halo_frames(r, &K)) exit(1);
    if (a->halo >= 0 && K > 0) K = a->halo;
    if (hipMalloc(&d_in, fb * a->B) != hipSuccess || hipMalloc(&d_out, fb * a->B) != hipSuccess ||
        hipMalloc(&d_next, fb) != hipSuccess || (K > 0 && hipMalloc(&d_halo, fb * K) != hipSuccess)) {
        fprintf(stderr, "rank %d: hipMalloc failed\n", a->rank);
        exit(1);
    }
    hipStream_t s = (hipStream_t)mm_stream(h);
    for (int st = 0; st < steps; ++st) {
        const int t0 = st * a->world * a->B + a->rank * a->B;
        const int more = st + 1 < steps;
        if ((rc = mm_synth_frames(d_in, a->W, a->H, t0, a->B, 0x5EED0000ull, 0, s)) ||
            (more && (rc = mm_synth_frames(d_next, a->W, a->H, t0 + a->world * a->B + a->B - 1, 1,
                                           0x5EED0000ull, 0, s)))) {
            fprintf(stderr, "rank %d: mm_synth_frames: %s\n", a->rank, mm_strerror(rc));
            exit(1);
        }
        const int hk = t0 < K ? t0 : K;   /* IIR: the warm-up halo before the chunk */
        if (hk && (rc = mm_synth_frames(d_halo, a->W, a->H, t0 - hk, hk, 0x5EED0000ull, 0, s))) exit(1);
        if ((rc = K > 0 ? mm_ring_step_halo(r, st, d_halo, hk, d_in, d_out, s)
                        : mm_ring_step(r, st, d_in, d_out, more ? d_next : NULL, s))) {
            fprintf(stderr, "rank %d: mm_ring_step: %s (%s)\n", a->rank, mm_strerror(rc), mm_ring_last_error());
            exit(1);
        }
        if (a->d_all && hipMemcpyAsync(a->d_all + fb * (size_t)t0, d_out, fb * a->B, hipMemcpyDeviceToDevice, s) !=
                            hipSuccess) {
            fprintf(stderr, "rank %d: keep outputs\n", a->rank);
            exit(1);
        }
        if (a->checksum) {
            if (hipStreamSynchronize(s) != hipSuccess ||
                hash_frames((const unsigned char *)d_out, fb, a->B, a->hashes + t0)) {
                fprintf(stderr, "rank %d: readback failed\n", a->rank);
                exit(1);
            }
        }
    }
    if (hipStreamSynchronize(s) != hipSuccess) { fprintf(stderr, "rank %d: stream\n", a->rank); exit(1); }
    mm_ring_destroy(r);
    mm_destroy(h);
    hipFree(d_in);
    hipFree(d_out);
    hipFree(d_next);
    hipFree(d_halo);
    a->rc = 0;
    return NULL;
}

/* --compare: the same stream through one handle in calls of B frames, frame
 * by frame against the ring's outputs: "cmp t maxabs ndiff" per frame and a
 * summary line (the IIR halo's tolerance, tests/test_ring_c.py) */
static int compare_single(const mm_params *p, int W, int H, int F, int B, int dev, const unsigned char *d_all)
{
    const size_t fb = (size_t)W * H * 4;
    mm_handle *h = NULL;
    void *d_in = NULL, *d_out = NULL;
    unsigned char *a = (unsigned char *)malloc(fb), *b = (unsigned char *)malloc(fb);
    if (!a || !b) return 1;
    CHECK(mm_create(W, H, p, dev, &h));
    CHECK(mm_set_batch(h, B));
    if (hipMalloc(&d_in, fb * B) != hipSuccess || hipMalloc(&d_out, fb * B) != hipSuccess) return 1;
    hipStream_t s = (hipStream_t)mm_stream(h);
    long long ndiff_all = 0;
    int max_all = 0;
    for (int f0 = 0; f0 < F; f0 += B) {
        CHECK(mm_synth_frames(d_in, W, H, f0, B, 0x5EED0000ull, 0, s));
        CHECK(mm_process_stream(h, d_in, d_out, B, g_fmt, s));
        if (hipStreamSynchronize(s) != hipSuccess) return 1;
        for (int k = 0; k < B; ++k) {
            if (hipMemcpy(a, (unsigned char *)d_out + fb * k, fb, hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(b, d_all + fb * (size_t)(f0 + k), fb, hipMemcpyDeviceToHost) != hipSuccess)
                return 1;
            int mx = 0;
            long long nd = 0;
            for (size_t i = 0; i < fb; ++i) {
                const int d = a[i] > b[i] ? a[i] - b[i] : b[i] - a[i];
                if (d) {
                    ++nd;
                    if (d > mx) mx = d;
                }
            }
            printf("cmp %d %d %lld\n", f0 + k, mx, nd);
            ndiff_all += nd;
            if (mx > max_all) max_all = mx;
        }
    }
    printf("compare frames %d maxabs %d ndiff %lld values %lld\n", F, max_all, ndiff_all, (long long)fb * F);
    mm_destroy(h);
    hipFree(d_in);
    hipFree(d_out);
    free(a);
    free(b);
    return 0;
}

static int run_ring_local(const mm_params *p, int W, int H, int F, int B, int dev, int world, int checksum,
                          int halo, int compare)
{
    if (world < 1 || world > 64 || F % (world * B) != 0) {
        fprintf(stderr, "--ring-local: need 1 <= G <= 64 and frames a multiple of G * batch\n");
        return 2;
    }
    mm_ring_hub *hub = NULL;
    if (mm_ring_hub_create(world, &hub)) return 1;
    uint64_t *hashes = (uint64_t *)calloc((size_t)F, sizeof(uint64_t));
    local_rank *ranks = (local_rank *)calloc((size_t)world, sizeof(local_rank));
    pthread_t *th = (pthread_t *)calloc((size_t)world, sizeof(pthread_t));
    if (!hashes || !ranks || !th) return 1;
    unsigned char *d_all = NULL;
    if (compare) {
        if (hipSetDevice(dev) != hipSuccess || hipMalloc((void **)&d_all, (size_t)W * H * 4 * (size_t)F) != hipSuccess) {
            fprintf(stderr, "--compare: hipMalloc of %d frames failed\n", F);
            return 1;
        }
    }
    for (int g = 0; g < world; ++g) {
        local_rank *a = &ranks[g];
        a->hub = hub;
        a->p = p;
        a->W = W; a->H = H; a->F = F; a->B = B; a->dev = dev;
        a->world = world; a->rank = g; a->checksum = checksum;
        a->hashes = hashes;
        a->halo = halo;
        a->d_all = d_all;
        if (pthread_create(&th[g], NULL, local_rank_main, a) != 0) {
            fprintf(stderr, "pthread_create failed\n");
            exit(1);
        }
    }
    int rc = 0;
    for (int g = 0; g < world; ++g) {
        pthread_join(th[g], NULL);
        rc |= ranks[g].rc;
    }
    if (!rc && checksum)
        for (int t = 0; t < F; ++t) printf("frame %d %llu\n", t, (unsigned long long)hashes[t]);
    printf("ring-local world %d  steps %d  chunk %d\n", world, F / (world * B), B);
    if (!rc && compare) rc = compare_single(p, W, H, F, B, dev, d_all);
    if (d_all) hipFree(d_all);
    mm_ring_hub_destroy(hub);
    free(hashes);
    free(ranks);
    free(th);
    return rc;
}

/* ---- the input-format options: one row each ------------------------------ */
typedef void (*pack_fn)(int W, int H, const void *from, void *to);
typedef int (*whdr_fn)(FILE *f, int W, int H, int fps_num, int fps_den, int depth);
typedef int (*wframe_fn)(FILE *f, int W, int H, int depth, const void *planes);
#define PACK_FN(name, call) static void name(int W, int H, const void *a, void *b) { call; }
PACK_FN(pack_nv12, y4m_420_to_nv12(W, H, a, b))
PACK_FN(unpack_nv12, y4m_nv12_to_420(W, H, a, b))
PACK_FN(pack_p010, y4m_420p10_to_p010(W, H, a, b))
PACK_FN(unpack_p010, y4m_p010_to_420p10(W, H, a, b))
PACK_FN(pack_yuy2, y4m_422_to_packed(W, H, a, b, 0))
PACK_FN(unpack_yuy2, y4m_packed_to_422(W, H, a, b, 0))
PACK_FN(pack_uyvy, y4m_422_to_packed(W, H, a, b, 1))
PACK_FN(unpack_uyvy, y4m_packed_to_422(W, H, a, b, 1))
PACK_FN(pack_y210, y4m_422p10_to_y210(W, H, a, b))
PACK_FN(unpack_y210, y4m_y210_to_422p10(W, H, a, b))
/* (the container has no v210 tag: the C422p10 planes are packed on the host, rows at the standard pitch) */
PACK_FN(pack_v210, (void)v210_pack_422p10(W, H, a, b, v210_pitch(W)))
PACK_FN(unpack_v210, (void)v210_unpack_422p10(W, H, a, v210_pitch(W), b))
/* the .y4m writers of one chroma type under one signature (mono's own take the depth) */
#define WRITE_FNS(name, hdr, frame)                                                        \
    static int whdr_##name(FILE *f, int W, int H, int n, int d, int depth) { (void)depth; return hdr(f, W, H, n, d); } \
    static int wframe_##name(FILE *f, int W, int H, int depth, const void *p) { (void)depth; return frame(f, W, H, p); }
WRITE_FNS(444, y4m_write_header, y4m_write_frame)
WRITE_FNS(420, y4m_write_header_420, y4m_write_frame_420)
WRITE_FNS(420p10, y4m_write_header_420p10, y4m_write_frame_420p10)
WRITE_FNS(422, y4m_write_header_422, y4m_write_frame_422)
WRITE_FNS(422p10, y4m_write_header_422p10, y4m_write_frame_422p10)

typedef struct {
    const char *name;     /* the flag */
    int chroma, depth;    /* the .y4m it takes: chroma type (-1: none) and bit depth (0: any, the code follows it) */
    int raw;              /* any other extension: the raw frames (else a .y4m only) */
    int fmt, fmt_full;    /* the frame format; with --full-range */
    int ycc;              /* Y'CbCr: takes --matrix and --full-range, needs even sizes */
    int views;            /* goes with --show-magnitude / --show-phase */
    int decode;           /* goes with --out-rgba8 */
    const char *needs;    /* the input it needs, in the refusal's words */
    pack_fn pack, unpack; /* .y4m planes -> frame and back (NULL: the frame goes as it lies in the file) */
    whdr_fn whdr;         /* the .y4m it writes */
    wframe_fn wframe;
} in_opt;
static const in_opt k_in_opts[] = {
    {"--nv12", Y4M_420, 8, 0, MM_NV12, MM_NV12_FULL, 1, 0, 1, "an 8-bit 4:2:0 .y4m input (-i, C420)",
     pack_nv12, unpack_nv12, whdr_420, wframe_420},
    {"--p010", Y4M_420, 10, 0, MM_P010, MM_P010_FULL, 1, 0, 1, "a 10-bit input (C420p10), a 4:2:0 .y4m (-i)",
     pack_p010, unpack_p010, whdr_420p10, wframe_420p10},
    {"--i420", Y4M_420, 8, 1, MM_I420, MM_I420_FULL, 1, 0, 0,
     "an 8-bit 4:2:0 .y4m input (-i, C420; a C420p10 stream takes --p010 or --i010), or raw I420 frames under any other extension",
     NULL, NULL, whdr_420, wframe_420},
    {"--i010", Y4M_420, 10, 1, MM_I010, MM_I010_FULL, 1, 0, 0,
     "a 10-bit 4:2:0 .y4m input (-i, C420p10; an 8-bit C420 stream takes --i420), or raw I010 frames under any other extension",
     NULL, NULL, whdr_420p10, wframe_420p10},
    {"--mono", Y4M_MONO, 0, 0, MM_Y8, MM_Y8, 0, 1, 0, "a mono .y4m input (-i, Cmono / Cmono10 / Cmono12 / Cmono16)",
     NULL, NULL, y4m_write_header_mono, y4m_write_frame_mono},
    {"--yuy2", Y4M_422, 8, 0, MM_YUY2, MM_YUY2_FULL, 1, 0, 0, "an 8-bit 4:2:2 .y4m input (-i, C422)",
     pack_yuy2, unpack_yuy2, whdr_422, wframe_422},
    {"--uyvy", Y4M_422, 8, 0, MM_UYVY, MM_UYVY_FULL, 1, 0, 0, "an 8-bit 4:2:2 .y4m input (-i, C422)",
     pack_uyvy, unpack_uyvy, whdr_422, wframe_422},
    {"--y210", Y4M_422, 10, 0, MM_Y210, MM_Y210_FULL, 1, 0, 0, "a 10-bit 4:2:2 .y4m input (-i, C422p10)",
     pack_y210, unpack_y210, whdr_422p10, wframe_422p10},
    {"--v210", Y4M_422, 10, 0, MM_V210, MM_V210_FULL, 1, 0, 0, "a 10-bit 4:2:2 .y4m input (-i, C422p10)",
     pack_v210, unpack_v210, whdr_422p10, wframe_422p10},
    /* (a stream of binary PPM images: its own reader and writer, main's ppm branches; --bgr) */
    {"--ppm", -1, 8, 1, MM_RGB24, MM_RGB24, 0, 0, 0,
     "a binary PPM stream as input (-i, P6, maxval 255) and writes one (-o): no .y4m on either side", NULL, NULL, NULL, NULL},
};
static const in_opt *const k_opt_nv12 = &k_in_opts[0], *const k_opt_ppm = &k_in_opts[9];

/* The option a .y4m input cannot do without: the host converts 8-bit 4:2:0,
 * 4:4:4 and mono to RGBA8 and nothing else, and no bit depth silently. */
static const char *y4m_needs(const y4m_info *yi, int depth)
{
    if (yi->chroma == Y4M_422) return depth == 10 ? "--y210 or --v210" : "--yuy2 or --uyvy";
    if (depth == 8) return NULL;
    return yi->chroma == Y4M_MONO ? "--mono" : "--p010";
}

/* --ppm --bgra: an image's R G B pixels widened in place to B G R 255
 * (MM_BGRA8; the buffer holds 4 bytes per pixel), and back, the alpha dropped */
static void ppm_widen_bgra(unsigned char *p, size_t npx)
{
    for (size_t i = npx; i-- > 0;) {
        const unsigned char r = p[3 * i], g = p[3 * i + 1], b = p[3 * i + 2];
        p[4 * i] = b, p[4 * i + 1] = g, p[4 * i + 2] = r, p[4 * i + 3] = 255;
    }
}
static void ppm_narrow_bgra(unsigned char *p, size_t npx)
{
    for (size_t i = 0; i < npx; ++i) {
        const unsigned char b = p[4 * i], g = p[4 * i + 1], r = p[4 * i + 2];
        p[3 * i] = r, p[3 * i + 1] = g, p[3 * i + 2] = b;
    }
}

#define REFUSE(...) do { fprintf(stderr, __VA_ARGS__); return 2; } while (0)

int main(int argc, char **argv)
{
    int W = 1920, H = 1080, F = 300, L = 5, B = 30, dev = 0;
    int full_range = 0, standard = 0, show_mag = 0, show_phase = 0, checksum = 0;
    int ring_world = 0, ring_rank = 0, ring_local = 0, orientations = 1, iir = 0, halo = -1, compare = 0;
    int srgb = 0, bgr = 0, bgra = 0, out_rgba8 = 0, out_bgra8 = 0, out_nv12 = 0;
    const char *lanes_arg = NULL, *drop_arg = NULL, *hold_arg = NULL;
    const in_opt *in = NULL;  /* the input-format option: one at most */
    const char *matrix_arg = NULL;
    const char *surf_arg = NULL;
    float S = 25.0f;
    const char *in_path = NULL, *out_path = NULL, *ring_id_path = NULL;
    for (int i = 1; i < argc; ++i) {
        const char *a = argv[i];
        const in_opt *o = NULL;
        for (size_t k = 0; k < sizeof k_in_opts / sizeof *k_in_opts; ++k)
            if (!strcmp(a, k_in_opts[k].name)) o = &k_in_opts[k];
        if (o) {
            if (in && in != o) REFUSE("%s does not go with %s (one input format)\n", in->name, o->name);
            in = o;
            continue;
        }
        if (!strcmp(a, "--full-range")) { full_range = 1; continue; }
        if (!strcmp(a, "--srgb")) { g_fmt = MM_RGBA8_SRGB; srgb = 1; continue; }
        if (!strcmp(a, "--bgr")) { bgr = 1; continue; }
        if (!strcmp(a, "--bgra")) { bgra = 1; continue; }
        if (!strcmp(a, "--out-rgba8")) { out_rgba8 = 1; continue; }
        if (!strcmp(a, "--out-bgra8")) { out_bgra8 = 1; continue; }
        if (!strcmp(a, "--out-nv12")) { out_nv12 = 1; continue; }
        if (!strcmp(a, "--standard")) { standard = 1; continue; }
        if (!strcmp(a, "--show-magnitude")) { show_mag = 1; continue; }
        if (!strcmp(a, "--show-phase")) { show_phase = 1; continue; }
        if (!strcmp(a, "--checksum")) { checksum = 1; continue; }
        if (!strcmp(a, "--iir")) { iir = 1; continue; }
        if (!strcmp(a, "--compare")) { compare = 1; continue; }
        const char *v = i + 1 < argc ? argv[i + 1] : NULL;
        if (!v) { fprintf(stderr, "missing value for %s\n", a); return 2; }
        if (!strcmp(a, "-w")) W = atoi(v);
        else if (!strcmp(a, "-h")) H = atoi(v);
        else if (!strcmp(a, "-n")) F = atoi(v);
        else if (!strcmp(a, "-l")) L = atoi(v);
        else if (!strcmp(a, "-s")) S = (float)atof(v);
        else if (!strcmp(a, "-b")) B = atoi(v);
        else if (!strcmp(a, "-d")) dev = atoi(v);
        else if (!strcmp(a, "-i")) in_path = v;
        else if (!strcmp(a, "-o")) out_path = v;
        else if (!strcmp(a, "--ring-world")) ring_world = atoi(v);
        else if (!strcmp(a, "--ring-rank")) ring_rank = atoi(v);
        else if (!strcmp(a, "--ring-id")) ring_id_path = v;
        else if (!strcmp(a, "--ring-local")) ring_local = atoi(v);
        else if (!strcmp(a, "--orientations")) orientations = atoi(v);
        else if (!strcmp(a, "--halo")) halo = atoi(v);
        else if (!strcmp(a, "--surface-align")) surf_arg = v;
        else if (!strcmp(a, "--matrix")) matrix_arg = v;
        else if (!strcmp(a, "--lanes")) lanes_arg = v;
        else if (!strcmp(a, "--lane-drop")) drop_arg = v;
        else if (!strcmp(a, "--hold")) hold_arg = v;
        else { fprintf(stderr, "unknown option %s\n", a); return 2; }
        ++i;
    }
    if (B < 1) B = 1;
    /* Every refusal below comes before the output file is opened and before the
     * device is touched.  First what the options say by themselves. */
    const int views = show_mag || show_phase, ring = ring_local > 0 || ring_world > 0;
    const int p_ppm = in == k_opt_ppm;
    /* --out-bgra8 is --out-rgba8 with MM_BGRA8 as the output code: one set of rules */
    if (out_rgba8 && out_bgra8) REFUSE("--out-rgba8 does not go with --out-bgra8 (one output format)\n");
    const char *out4 = out_bgra8 ? "--out-bgra8" : "--out-rgba8";
    out_rgba8 |= out_bgra8;
    if (in) {
        const char *bad = srgb ? "--srgb" : ring ? "the ring modes (they take RGBA frames)"
                          : views && !in->views ? "the debug views" : out_nv12 ? "--out-nv12 (it takes the RGBA8 input path)"
                          : out_rgba8 && !in->decode ? (out_bgra8 ? "--out-bgra8 (it takes --nv12 or --p010)"
                                                                   : "--out-rgba8 (it takes --nv12 or --p010)")
                          : matrix_arg && !in->ycc ? "--matrix (there is no matrix)"
                          : full_range && !in->ycc ? "--full-range (there is no range)" : NULL;
        if (bad) REFUSE("%s does not go with %s\n", in->name, bad);
        if (!in_path) REFUSE("%s needs an input (-i): %s\n", in->name, in->needs);
    }
    if (bgr && !p_ppm) REFUSE("--bgr needs --ppm\n");
    if (bgra && !p_ppm) REFUSE("--bgra needs --ppm\n");
    if (bgra && bgr) REFUSE("--bgra does not go with --bgr (one byte order)\n");
    /* different formats in and out (mm_process_stream_convert) */
    if (out_rgba8 && out_nv12) REFUSE("%s does not go with --out-nv12\n", out4);
    if (out_rgba8 && !in) REFUSE("%s needs --nv12 or --p010 (the default path takes and gives RGBA8)\n", out4);
    if (out_nv12 && (srgb || views || ring))
        REFUSE("--out-nv12 takes the RGBA8 input path: not with --srgb, the debug views or the ring modes\n");
    if (matrix_arg && !(in && in->ycc) && !out_nv12)
        REFUSE("--matrix needs --nv12, --p010, --yuy2, --uyvy, --y210, --v210, --i420, --i010 or --out-nv12 (the RGBA conversion of a .y4m is BT.601)\n");
    if (matrix_arg && strcmp(matrix_arg, "601") && strcmp(matrix_arg, "709") && strcmp(matrix_arg, "2020"))
        REFUSE("--matrix takes 601, 709 or 2020, not %s (%s)\n", matrix_arg, in ? in->name : "--out-nv12");
    if (surf_arg && ring) REFUSE("--surface-align does not go with the ring modes (they take tight frames)\n");
    /* several live streams per call (mm_process_lanes) */
    const int M = lanes_arg ? atoi(lanes_arg) : 0;
    if (lanes_arg && (M < 1 || M > MM_LANES_MAX)) REFUSE("--lanes takes 1 .. %d, not %s\n", MM_LANES_MAX, lanes_arg);
    if (M && (orientations > 1 || iir || views || ring))
        REFUSE("--lanes does not go with --orientations / --iir, the debug views or the ring modes\n");
    if (M) B = M;
    /* frames that never arrived (mm_process_lanes_mask) */
    lane_drop *drops = NULL;
    int ndrops = 0;
    if (drop_arg) {
        if (!M) REFUSE("--lane-drop needs --lanes\n");
        if (!in_path || checksum || out_rgba8 || out_nv12)
            REFUSE("--lane-drop needs an input file (-i) and does not go with --checksum, --out-rgba8 or --out-nv12\n");
        drops = parse_lane_drops(drop_arg, M, &ndrops);
        if (!drops) REFUSE("--lane-drop takes L:T[,L:T...] with lanes 0 .. %d, not %s\n", M - 1, drop_arg);
    }
    /* a held reference frame (mm_set_hold) */
    char *hold_end = NULL;
    const long hold_l = hold_arg ? strtol(hold_arg, &hold_end, 10) : -1;
    const int hold_R = hold_arg && isdigit((unsigned char)hold_arg[0]) && !*hold_end && hold_l <= 1000000000L ? (int)hold_l : -1;
    if (hold_arg && hold_R < 0)
        REFUSE("--hold takes 0 (the first frame is the reference throughout) or R > 0 (a new reference every R frames), not %s\n", hold_arg);
    if (hold_arg && (orientations > 1 || iir || views || ring))
        REFUSE("--hold does not go with --orientations / --iir, the debug views or the ring modes\n");
    if (ring_local > 0 && (in_path || out_path)) REFUSE("--ring-local needs a synthetic stream\n");
    if (ring_world > 0 && ring_local <= 0 && (!ring_id_path || in_path || out_path))
        REFUSE("--ring-world needs --ring-id and a synthetic stream\n");
    /* ... then what the input says: the container and the geometry */
    FILE *fi = in_path ? fopen(in_path, "rb") : NULL;
    if (in_path && !fi) { fprintf(stderr, "cannot open file\n"); return 1; }
    const int y4m_in = in_path && ends_with(in_path, ".y4m");
    const int y4m_out = out_path && ends_with(out_path, ".y4m");
    if (out_bgra8 && y4m_out) REFUSE("--out-bgra8 writes raw B G R A frames, no .y4m (the .y4m writer takes RGBA8: --out-rgba8)\n");
    y4m_info yi = {0};
    yi.fps_num = 25;
    yi.fps_den = 1;
    int depth = 8;
    if (y4m_in) {
        if (y4m_read_header_ext(fi, &yi, &depth)) { fprintf(stderr, "%s: unsupported Y4M\n", in_path); return 1; }
        W = yi.width;
        H = yi.height;
    }
    const char *hint = y4m_in ? y4m_needs(&yi, depth) : NULL;
    if (in && ((y4m_in ? yi.chroma != in->chroma || (in->depth && depth != in->depth) : !in->raw) || (p_ppm && y4m_out))) {
        if (hint) REFUSE("%s needs %s; %s needs %s\n", in->name, in->needs, in_path, hint);
        REFUSE("%s needs %s\n", in->name, in->needs);
    }
    if (!in && hint)
        REFUSE("%s is a %d-bit %s stream: it needs %s (it is never converted on the host)\n", in_path, depth,
               yi.chroma == Y4M_422 ? "4:2:2" : yi.chroma == Y4M_MONO ? "mono" : "4:2:0", hint);
    /* --ppm: a stream of binary PPM images is a stream of MM_RGB24 frames */
    ppm_info pi = {0, 0};
    int ppm_pending = 0;   /* the first image's header is read, its pixels are not */
    if (p_ppm) {
        const int rc = ppm_read_header(fi, &pi);
        if (rc) {
            fprintf(stderr, "%s: %s\n", in_path,
                    rc == PPM_EOF ? "empty file" : rc == PPM_ERR_MAGIC ? "not a binary PPM (P6)"
                    : rc == PPM_ERR_MAXVAL ? "maxval is not 255" : "malformed PPM header");
            return 1;
        }
        W = pi.width;
        H = pi.height;
        ppm_pending = 1;
    }
    if (((in && in->ycc) || out_nv12) && ((W | H) & 1))
        REFUSE("%s needs even width and height (%dx%d)\n", in ? in->name : "--out-nv12", W, H);
    /* the frame format: the row's code (mono: by the header's depth), the
     * output side's with --out-rgba8 / --out-nv12; --matrix's bit goes on the
     * Y'CbCr side (--out-nv12: it names the output code, the input is RGBA8) */
    const int mbit = !matrix_arg ? 0 : !strcmp(matrix_arg, "709") ? MM_MATRIX_BT709
                     : !strcmp(matrix_arg, "2020") ? MM_MATRIX_BT2020 : 0;
    if (in)
        g_fmt = !in->depth ? (depth == 8 ? MM_Y8 : depth == 10 ? MM_Y10 : depth == 12 ? MM_Y12 : MM_Y16)
                : p_ppm && bgr ? MM_BGR24 : p_ppm && bgra ? MM_BGRA8 : (full_range ? in->fmt_full : in->fmt) | mbit;
    const int o_fmt = out_nv12 ? (full_range ? MM_NV12_FULL : MM_NV12) | mbit : out_bgra8 ? MM_BGRA8 : out_rgba8 ? MM_RGBA8 : g_fmt;
    const int convert = o_fmt != g_fmt;
    /* what a .y4m output holds, and how its frames are made: the input
     * option's, --out-nv12: --nv12's, --out-rgba8 or no option: 4:4:4 from RGBA8 */
    const in_opt *wr = out_nv12 ? k_opt_nv12 : out_rgba8 ? NULL : in;
    if (M) {
        /* --lanes: whole ticks only.  The frames a file holds (-n at most) are
         * counted by reading it once; the run then starts where this started. */
        int count = F;
        if (fi) {
            size_t cb = (size_t)W * H * 4;
            if (in && mm_frame_bytes(W, H, g_fmt, &cb) != MM_OK) cb = 0;
            if (y4m_in && y4m_frame_bytes_depth(&yi, depth) > cb) cb = y4m_frame_bytes_depth(&yi, depth);
            unsigned char *tmp = cb ? (unsigned char *)malloc(cb) : NULL;
            const long pos = ftell(fi);
            ppm_info pc = pi;
            if (!tmp || pos < 0) { fprintf(stderr, "cannot count the frames of %s\n", in_path); return 1; }
            for (count = 0; count < F; ++count) {
                int more;
                if (y4m_in) more = y4m_read_frame_depth(fi, &yi, depth, tmp) > 0;
                else if (p_ppm) more = (count == 0 ? ppm_read_pixels(fi, &pc, tmp) : ppm_read_next(fi, &pc, tmp)) == 0;
                else more = fread(tmp, cb, 1, fi) == 1;
                if (!more) break;
            }
            free(tmp);
            if (fseek(fi, pos, SEEK_SET)) { fprintf(stderr, "cannot rewind %s\n", in_path); return 1; }
        }
        if (count % M) REFUSE("--lanes %d needs a multiple of %d frames, not %d\n", M, M, count);
        F = count;
    }
    FILE *fo = out_path ? fopen(out_path, "wb") : NULL;
    if (out_path && !fo) { fprintf(stderr, "cannot open file\n"); return 1; }
    mm_params p;
    mm_params_default(&p);
    p.levels = L;
    p.phase_scale = S;
    p.mode = standard ? MM_MODE_STANDARD : orientations > 1 ? MM_MODE_STEERABLE : MM_MODE_PYRAMID;
    p.orientations = orientations;
    p.temporal_filter = iir ? MM_FILTER_IIR : MM_FILTER_DIFF;
    p.show_magnitude = show_mag;
    p.show_phase = show_phase;
    if (ring_local > 0) return run_ring_local(&p, W, H, F, B, dev, ring_local, checksum, halo, compare);
    /* mm_create runs on `dev` and gives the caller's current device back:
     * this program's own buffers, events and default stream must be on `dev`
     * too (before its first HIP allocation) */
    if (hipSetDevice(dev) != hipSuccess) {
        fprintf(stderr, "hipSetDevice(%d) failed\n", dev);
        return 1;
    }
    mm_handle *h = NULL;
    CHECK(mm_create(W, H, &p, dev, &h));
    int N = 0;
    mm_padded_size(h, &N);
    printf("Original: %dx%d, Padded: %dx%d\n", W, H, N, N);   /* .cs:304 */
    if (M) CHECK(mm_set_lanes(h, M));
    if (ring_world > 0) {
        CHECK(mm_set_batch(h, B));
        const int rc = run_ring(h, W, H, F, B, dev, ring_world, ring_rank, ring_id_path, checksum, halo);
        mm_destroy(h);
        return rc;
    }

    size_t fb = (size_t)W * H * 4;
    if (in) CHECK(mm_frame_bytes(W, H, g_fmt, &fb));
    /* --surface-align: the frames the operator sees live in `lay` surfaces
     * (d_in, d_out); d_tin / d_tout are tight device frames for the synthetic
     * source and for the checksums and files */
    size_t fbo = fb;   /* ... and of the output side */
    if (convert) CHECK(mm_frame_bytes(W, H, o_fmt, &fbo));
    mm_surface tight, lay, otight, olay;
    CHECK(mm_surface_tight(W, H, g_fmt, &tight));
    CHECK(mm_surface_tight(W, H, o_fmt, &otight));
    lay = tight;
    olay = otight;
    if (surf_arg) {
        unsigned long long pa = 0;
        int ra = 0, rc;
        if (sscanf(surf_arg, "%llu,%d", &pa, &ra) != 2 ||
            (rc = mm_surface_aligned(W, H, g_fmt, (size_t)pa, ra, &lay)) != MM_OK ||
            (rc = mm_surface_aligned(W, H, o_fmt, (size_t)pa, ra, &olay)) != MM_OK) {
            fprintf(stderr, "--surface-align %s: want P,R with P a multiple of the format's unit "
                            "(pixel size; NV12 2, P010 and 4:2:2 4, Y210 8, v210 16, mono: the sample size, --ppm and --i420: 1, --i010: 2; --i420: an even pitch, --i010: a multiple of 4) and R >= 1 (4:2:0: even)\n", surf_arg);
            return 2;
        }
        printf("surfaces: pitch %zu  chroma offset %zu  frame stride %zu\n", lay.pitch, lay.chroma_offset,
               lay.frame_stride);
    }
    void *d_in = NULL, *d_out = NULL, *d_tin = NULL, *d_tout = NULL;
    if (hipMalloc(&d_in, lay.frame_stride * B) != hipSuccess || hipMalloc(&d_out, olay.frame_stride * B) != hipSuccess ||
        (surf_arg && (hipMalloc(&d_tin, fb * B) != hipSuccess || hipMalloc(&d_tout, fbo * B) != hipSuccess))) {
        fprintf(stderr, "hipMalloc failed\n");
        return 1;
    }
    /* (a tight v210 frame has row padding, which nothing writes: zeroed once, so
     * that checksums and raw files of whole tight frames are those of every run) */
    if ((g_fmt & MM_PACK_V210) &&
        (hipMemset(d_in, 0, lay.frame_stride * B) != hipSuccess || hipMemset(d_out, 0, olay.frame_stride * B) != hipSuccess ||
         (surf_arg && (hipMemset(d_tin, 0, fb * B) != hipSuccess || hipMemset(d_tout, 0, fbo * B) != hipSuccess)))) {
        fprintf(stderr, "hipMemset failed\n");
        return 1;
    }
    hipStream_t s = (hipStream_t)mm_stream(h);
    unsigned char *host = (fi || fo) ? (unsigned char *)calloc((size_t)B, fb > fbo ? fb : fbo) : NULL;
    /* --lane-drop: a tick's input frames, kept for its dropped slots of the output */
    unsigned char *kept = ndrops && fo ? (unsigned char *)malloc((size_t)B * fb) : NULL;
    if (ndrops && fo && !kept) { fprintf(stderr, "out of memory\n"); return 1; }
    unsigned char *planes = (y4m_in || y4m_out)
        ? (unsigned char *)malloc(y4m_in ? (y4m_frame_bytes_depth(&yi, depth) > 3 * (size_t)W * H
                                               ? y4m_frame_bytes_depth(&yi, depth) : 3 * (size_t)W * H)
                                         : 3 * (size_t)W * H)
        : NULL;
    /* (planes: 3 W H bytes hold a C420p10 frame, 2 bytes per sample, exactly; a
     * C422p10 frame takes 4 W H) */
    if (y4m_out && (wr ? wr->whdr : whdr_444)(fo, W, H, yi.fps_num, yi.fps_den, depth)) {
        fprintf(stderr, "write failed\n");
        return 1;
    }

    double t_proc = 0.0;
    int done = 0;
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    while (done < F) {
        int n = F - done < B ? F - done : B;
        const uint64_t mask = M ? tick_mask(drops, ndrops, M, done / M) : 0;
        if (fi && y4m_in) {
            int got = 0;
            for (; got < n; ++got) {
                /* (no pack function: the file's planes are the frame, read straight into place) */
                unsigned char *frame = host + fb * got;
                const int r = y4m_read_frame_depth(fi, &yi, depth, in && !in->pack ? frame : planes);
                if (r < 0) { fprintf(stderr, "%s: malformed frame\n", in_path); return 1; }
                if (r == 0) break;
                if (in && in->pack) in->pack(W, H, planes, frame);
                /* (--out-nv12: --full-range names the output code, the input is limited range) */
                else if (!in) y4m_to_rgba(&yi, planes, frame, out_nv12 ? 0 : full_range);
            }
            if (got == 0) break;
            n = got;
            if (surf_copy_mask(d_in, &lay, host, &tight, W, H, n, M ? mask : ~0ull, hipMemcpyHostToDevice, s)) return 1;
        } else if (fi && p_ppm) {
            /* images of the first one's size, as they lie (--bgr: R and B swapped) */
            int got = 0;
            for (; got < n; ++got) {
                const int r = ppm_pending ? ppm_read_pixels(fi, &pi, host + fb * got)
                                          : ppm_read_next(fi, &pi, host + fb * got);
                ppm_pending = 0;
                if (r == PPM_EOF) break;
                if (r) {
                    fprintf(stderr, "%s: %s\n", in_path,
                            r == PPM_ERR_TRUNCATED ? "truncated frame"
                            : r == PPM_ERR_SIZE    ? "a frame's size differs from the first's"
                            : r == PPM_ERR_MAXVAL  ? "maxval is not 255"
                            : r == PPM_ERR_MAGIC   ? "not a binary PPM (P6)" : "malformed PPM header");
                    return 1;
                }
                if (bgr) ppm_swap_rb(host + fb * got, (size_t)W * H);
                if (bgra) ppm_widen_bgra(host + fb * got, (size_t)W * H);
            }
            if (got == 0) break;
            n = got;
            if (surf_copy_mask(d_in, &lay, host, &tight, W, H, n, M ? mask : ~0ull, hipMemcpyHostToDevice, s)) return 1;
        } else if (fi) {
            size_t got = fread(host, fb, (size_t)n, fi);
            if (got == 0) break;
            n = (int)got;
            if (surf_copy_mask(d_in, &lay, host, &tight, W, H, n, M ? mask : ~0ull, hipMemcpyHostToDevice, s)) return 1;
        } else {
            CHECK(mm_synth_frames(surf_arg ? d_tin : d_in, W, H, done, n, 0x5EED0000ull, 0, s));
            if (surf_arg && surf_copy(d_in, &lay, d_tin, &tight, W, H, n, hipMemcpyDeviceToDevice, s)) return 1;
        }
        if (kept) memcpy(kept, host, (size_t)n * fb);   /* (`host` takes the output frames below) */
        hipEventRecord(e0, s);
        /* --hold R with --lanes: every lane holds; tick R, 2 R, ... runs with hold off */
        if (M && hold_R >= 0)
            CHECK(mm_set_lanes_hold(h, hold_R > 0 && done > 0 && (done / M) % hold_R == 0 ? 0 : M >= 64 ? ~0ull : (1ull << M) - 1));
        if (ndrops) CHECK(mm_process_lanes_mask(h, mask, d_in, &lay, d_out, &olay, s));
        else if (M) CHECK(mm_process_lanes(h, d_in, &lay, d_out, &olay, s));   /* (n == M: whole ticks) */
        else {
            /* --hold R: the calls are split at frames R, 2 R, ..., each of which
             * runs alone with hold off: it still pairs with the old reference and
             * leaves its own state behind as the new one */
            for (int k = 0, m; k < n; k += m) {
                const int g = done + k;
                const int reref = hold_R > 0 && g > 0 && g % hold_R == 0;
                m = reref ? 1 : n - k;
                if (hold_R > 0 && !reref && hold_R - g % hold_R < m) m = hold_R - g % hold_R;
                if (hold_R >= 0) CHECK(mm_set_hold(h, !reref));
                const unsigned char *ki = (const unsigned char *)d_in + lay.frame_stride * (size_t)k;
                unsigned char *ko = (unsigned char *)d_out + olay.frame_stride * (size_t)k;
                if (convert) CHECK(mm_process_stream_convert(h, ki, &lay, ko, &olay, m, s));
                else if (surf_arg) CHECK(mm_process_stream_surfaces(h, ki, &lay, ko, &lay, m, s));
                else CHECK(mm_process_stream(h, ki, ko, m, g_fmt, s));
            }
        }
        hipEventRecord(e1, s);
        hipEventSynchronize(e1);
        float ms = 0.0f;
        hipEventElapsedTime(&ms, e0, e1);
        if (done > 0) t_proc += ms * 1e-3;      /* first call holds the passthrough frame */
        const void *d_res = d_out;   /* the output frames, tight */
        if (surf_arg && (checksum || fo)) {
            if (surf_copy(d_tout, &otight, d_out, &olay, W, H, n, hipMemcpyDeviceToDevice, s) ||
                hipStreamSynchronize(s) != hipSuccess)
                return 1;
            d_res = d_tout;
        }
        if (checksum) print_checksums((const unsigned char *)d_res, fbo, n, done);
        if (fo) {
            hipMemcpy(host, d_res, fbo * n, hipMemcpyDeviceToHost);
            for (int k = 0; kept && k < n; ++k)   /* a dropped slot: its input, passed through (fbo == fb) */
                if (!((mask >> k) & 1)) memcpy(host + fb * k, kept + fb * k, fb);
            if (y4m_out) {
                for (int k = 0; k < n; ++k) {
                    /* (no unpack function: the frame is the file's planes) */
                    const unsigned char *frame = host + fbo * k;
                    if (wr && wr->unpack) wr->unpack(W, H, frame, planes);
                    else if (!wr) y4m_from_rgba(W, H, frame, planes, full_range);
                    if ((wr ? wr->wframe : wframe_444)(fo, W, H, depth, wr && !wr->unpack ? frame : planes)) {
                        fprintf(stderr, "write failed\n");
                        return 1;
                    }
                }
            } else if (p_ppm) {   /* the same container back */
                for (int k = 0; k < n; ++k) {
                    if (bgr) ppm_swap_rb(host + fb * k, (size_t)W * H);
                    if (bgra) ppm_narrow_bgra(host + fb * k, (size_t)W * H);
                    if (ppm_write_frame(fo, W, H, host + fb * k)) {
                        fprintf(stderr, "write failed\n");
                        return 1;
                    }
                }
            } else {
                fwrite(host, fbo, (size_t)n, fo);
            }
        }
        done += n;
    }
    int timed = done - (done > B ? B : done);
    if (timed > 0 && t_proc > 0)
        printf("frames %d  magnified fps %.1f  (%.3f ms/frame, %d frames per call)\n", done,
               timed / t_proc, 1e3 * t_proc / timed, B);
    else
        printf("frames %d\n", done);
    if (fi) fclose(fi);
    if (fo) fclose(fo);
    free(host);
    free(kept);
    free(drops);
    free(planes);
    hipFree(d_in);
    hipFree(d_out);
    hipFree(d_tin);
    hipFree(d_tout);
    mm_destroy(h);
    return 0;
}
