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
 *          [--yuy2] [--uyvy] [--y210] [--ppm [--bgr]] [--i420] [--i010] [--out-rgba8] [--out-nv12]
 *          [--standard] [--show-magnitude] [--show-phase]
 *          [--orientations O] [--iir] [--halo K] [--surface-align P,R]
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
 * --nv12: a 4:2:0 .y4m input goes to the device as it is stored, as MM_NV12
 * frames (MM_NV12_FULL with --full-range): the chroma planes are interleaved
 * on the way in and split on the way out (a C420 .y4m; any other extension:
 * the raw NV12 frames), and no colour arithmetic runs on the host.  Not with
 * --srgb, the debug views, the ring modes, 4:4:4 / mono input or odd sizes.
 * --p010: the same for a 10-bit 4:2:0 .y4m input (C420p10), sent as MM_P010
 * frames (MM_P010_FULL with --full-range): the chroma planes are interleaved
 * and every sample shifted left by 6 on the way in, the reverse on the way out
 * (a C420p10 .y4m; any other extension: the raw P010 frames).  Refused with
 * what --nv12 is refused with, and with --nv12.  Bit depths are never
 * converted silently: an 8-bit input with --p010 and a 10-bit input without it
 * are refused.
 * --matrix 601|709|2020 (default 601): the Y'CbCr matrix of an --nv12,
 * --p010, --yuy2, --uyvy or --y210 clip (HD content is BT.709, UHD BT.709 or BT.2020), OR-ed onto the
 * frame format as MM_MATRIX_BT709 / MM_MATRIX_BT2020.  A .y4m header has no
 * matrix tag, so files are the same whatever the value.  Only with --nv12,
 * --p010, --yuy2, --uyvy or --y210: the host's own RGBA conversion of a .y4m is BT.601.
 * --mono: a mono .y4m input (Cmono, Cmono10, Cmono12, Cmono16: a grayscale
 * camera's or ffmpeg's gray / gray10le / gray12le / gray16le frames) goes to
 * the device as it is stored, as MM_Y8 / MM_Y10 / MM_Y12 / MM_Y16 frames by the
 * header's depth: one sample per pixel each way, no conversion, odd sizes, the
 * standard and steerable modes and the debug views included.  The output is a
 * .y4m of the same Cmono* type (any other extension: the raw frames).  Refused
 * with a chroma-carrying input, with --nv12, --p010, --srgb, --matrix and
 * --full-range (there is no matrix and no range) and with the ring modes.
 * Without --mono a Cmono input is expanded to RGBA8 on the host, as before.
 * --yuy2 / --uyvy: an 8-bit 4:2:2 .y4m input (C422: a capture device's frames,
 * ffmpeg's yuv422p) goes to the device as packed macropixels, Y0 Cb Y1 Cr as
 * MM_YUY2 or Cb Y0 Cr Y1 as MM_UYVY (_FULL with --full-range, a matrix bit
 * with --matrix): the planes are interleaved on the way in and split on the
 * way out (a C422 .y4m, the same file for both flags; any other extension: the
 * raw packed frames), and no colour arithmetic runs on the host.  Refused
 * with --srgb, the debug views, the ring modes, --nv12, --p010, --mono, each
 * other, any other input and odd sizes.  A C422 input needs one of the two
 * flags: the host has no 4:2:2 to RGBA conversion.
 * --y210: a 10-bit 4:2:2 .y4m input (C422p10: planar, the code in the low 10
 * bits of each word; ffmpeg's yuv422p10le) goes to the device as MM_Y210
 * frames, words Y0 Cb Y1 Cr with the code << 6 (_FULL with --full-range, a
 * matrix bit with --matrix): the planes are interleaved and shifted on the way
 * in and split on the way out (a C422p10 .y4m; any other extension: the raw
 * Y210 frames), and no colour arithmetic runs on the host.  Refused with
 * --yuy2, --uyvy, --nv12, --p010, --mono, --srgb, the debug views, the ring
 * modes, any other input and odd sizes.  A C422p10 input needs --y210: it is
 * never converted on the host.
 * --ppm: the input (-i) is a stream of concatenated binary PPM images (P6,
 * maxval 255, one size: what ffmpeg -f image2pipe -vcodec ppm writes; host/ppm.h).
 * Its frames go to the device as MM_RGB24 as they lie, 3 bytes per pixel each
 * way, and -o gets the same container back.  --bgr swaps R and B on read and
 * on write and sends MM_BGR24 (the files are the run without it, byte for
 * byte).  Every size, -l, -s, -b, --standard and --surface-align as usual.
 * Refused with the other format options, --srgb, --matrix, --full-range, the
 * debug views, the ring modes and a .y4m on either side.
 * --i420: an 8-bit 4:2:0 .y4m input (C420) goes to the device as its frames lie
 * in the file, as MM_I420 frames (MM_I420_FULL with --full-range, a matrix bit
 * with --matrix): three planes, no interleave on the way in and no split on the
 * way out (a C420 .y4m; any other extension on either side: the raw I420
 * frames, -w/-h).  The output file is --nv12's, byte for byte.  -l, -s, -b,
 * --standard, --surface-align and --checksum as usual.  Refused with every
 * other format option (--nv12, --p010, --mono, --yuy2, --uyvy, --y210, --ppm),
 * --out-rgba8, --out-nv12, --srgb, the debug views, the ring modes, a .y4m
 * that is not 4:2:0 or is 10-bit, no input at all, and odd sizes.
 * --i010: a 10-bit 4:2:0 .y4m input (C420p10) goes to the device as its frames
 * lie in the file, as MM_I010 frames (MM_I010_FULL with --full-range, a matrix
 * bit with --matrix): three planes of words with the code in the low 10 bits,
 * no interleave and no shift on the way in, no split on the way out (a C420p10
 * .y4m; any other extension on either side: the raw I010 frames, -w/-h).  The
 * output file is --p010's, byte for byte.  -l, -s, -b, --standard,
 * --surface-align and --checksum as usual.  Refused with every other format
 * option (--nv12, --p010, --i420, --mono, --yuy2, --uyvy, --y210, --ppm),
 * --out-rgba8, --out-nv12, --srgb, the debug views, the ring modes, a .y4m
 * that is not 10-bit 4:2:0, no input at all, and odd sizes.
 * --surface-align P,R: the device frames, input and output, are held in
 * mm_surface_aligned(W, H, format, P, R) surfaces (256,16: a hardware
 * decoder's layout) and go through mm_process_stream_surfaces; for every input
 * format, --nv12, --p010, --yuy2, --uyvy and --y210 included.  Files and checksums are those of the
 * run without the flag, byte for byte.  Not with the ring modes.
 * --out-rgba8 (with --nv12 or --p010): decode on the way out.  The frames go
 * in as stored and raw MM_RGBA8 frames come out, through
 * mm_process_stream_convert: -o gets the raw RGBA8 frames, or, a .y4m, the 4:4:4
 * file the default RGBA8 path writes from them.  Refused without --nv12 /
 * --p010, with --out-nv12, and with whatever --nv12 / --p010 are refused with.
 * --out-nv12 (with the RGBA8 input path: a synthetic stream, raw RGBA8 frames,
 * or a .y4m the host expands as above): encode on the way out.  MM_RGBA8 frames
 * go in and NV12 frames come out: -o gets a C420 .y4m, or the raw NV12 frames.
 * --full-range and --matrix then name the OUTPUT code (MM_NV12_FULL, a matrix
 * bit) and nothing else: a .y4m input is expanded as BT.601 limited range.  Refused with --out-rgba8, every other format option (--nv12, --p010,
 * --mono, --yuy2, --uyvy, --y210, --ppm), --srgb, the debug views, the ring
 * modes and odd sizes.
 * With either, --surface-align lays out each side in its own format's
 * surface, and --checksum hashes the output frames, as usual.
 */
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mm.h"
#include "mm_ring.h"
#include "mm_ring_local.h"
#include "ppm.h"
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
    const size_t rb = t.pitch;   /* sample bytes of a row */
    if (dl->pitch == rb && sl->pitch == rb && dl->chroma_offset == t.chroma_offset &&
        sl->chroma_offset == t.chroma_offset && dl->chroma_pitch == t.chroma_pitch &&
        sl->chroma_pitch == t.chroma_pitch && dl->frame_stride == t.frame_stride &&
        sl->frame_stride == t.frame_stride)   /* tight on both sides: one copy */
        return hipMemcpyAsync(dst, src, t.frame_stride * (size_t)n, kind, s) != hipSuccess;
    for (int k = 0; k < n; ++k) {
        unsigned char *d = (unsigned char *)dst + dl->frame_stride * (size_t)k;
        const unsigned char *a = (const unsigned char *)src + sl->frame_stride * (size_t)k;
        if (hipMemcpy2DAsync(d, dl->pitch, a, sl->pitch, rb, (size_t)H, kind, s) != hipSuccess) return 1;
        /* (a chroma row: the luma row's bytes, or, three planes, half of them) */
        if (t.chroma_pitch && hipMemcpy2DAsync(d + dl->chroma_offset, dl->chroma_pitch, a + sl->chroma_offset,
                                               sl->chroma_pitch, t.chroma_pitch, (size_t)H / 2, kind, s) != hipSuccess)
            return 1;
        /* three planes: the Cr plane lies chroma_pitch x H/2 after the Cb plane */
        if ((dl->format & MM_PLANAR) &&
            hipMemcpy2DAsync(d + dl->chroma_offset + dl->chroma_pitch * ((size_t)H / 2), dl->chroma_pitch,
                             a + sl->chroma_offset + sl->chroma_pitch * ((size_t)H / 2), sl->chroma_pitch,
                             t.chroma_pitch, (size_t)H / 2, kind, s) != hipSuccess)
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

int main(int argc, char **argv)
{
    int W = 1920, H = 1080, F = 300, L = 5, B = 30, dev = 0;
    int full_range = 0, standard = 0, show_mag = 0, show_phase = 0, checksum = 0;
    int ring_world = 0, ring_rank = 0, ring_local = 0, orientations = 1, iir = 0, halo = -1, compare = 0;
    int nv12 = 0, p010 = 0, srgb = 0, mono = 0, yuy2 = 0, uyvy = 0, y210 = 0, ppm = 0, bgr = 0;
    int out_rgba8 = 0, out_nv12 = 0, i420 = 0, i010 = 0;
    const char *matrix_arg = NULL;
    const char *surf_arg = NULL;
    float S = 25.0f;
    const char *in_path = NULL, *out_path = NULL, *ring_id_path = NULL;
    for (int i = 1; i < argc; ++i) {
        const char *a = argv[i];
        if (!strcmp(a, "--full-range")) { full_range = 1; continue; }
        if (!strcmp(a, "--srgb")) { g_fmt = MM_RGBA8_SRGB; srgb = 1; continue; }
        if (!strcmp(a, "--nv12")) { nv12 = 1; continue; }
        if (!strcmp(a, "--p010")) { p010 = 1; continue; }
        if (!strcmp(a, "--mono")) { mono = 1; continue; }
        if (!strcmp(a, "--yuy2")) { yuy2 = 1; continue; }
        if (!strcmp(a, "--uyvy")) { uyvy = 1; continue; }
        if (!strcmp(a, "--y210")) { y210 = 1; continue; }
        if (!strcmp(a, "--ppm")) { ppm = 1; continue; }
        if (!strcmp(a, "--bgr")) { bgr = 1; continue; }
        if (!strcmp(a, "--i420")) { i420 = 1; continue; }
        if (!strcmp(a, "--i010")) { i010 = 1; continue; }
        if (!strcmp(a, "--out-rgba8")) { out_rgba8 = 1; continue; }
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
        else { fprintf(stderr, "unknown option %s\n", a); return 2; }
        ++i;
    }
    if (B < 1) B = 1;
    /* --i010 with another format option: refused before any file is opened */
    if (i010 && (nv12 || p010 || i420 || mono || yuy2 || uyvy || y210 || ppm || out_rgba8 || out_nv12 || srgb || show_mag ||
                 show_phase || ring_local > 0 || ring_world > 0)) {
        fprintf(stderr, "--i010 does not go with --nv12, --p010, --i420, --mono, --yuy2, --uyvy, --y210, --ppm, --out-rgba8, "
                        "--out-nv12, --srgb, the debug views or the ring modes\n");
        return 2;
    }
    if (i010 && !in_path) {
        fprintf(stderr, "--i010 needs an input (-i): a 10-bit 4:2:0 .y4m (C420p10) or raw I010 frames\n");
        return 2;
    }
    /* --i420 with another format option: refused before any file is opened */
    if (i420 && (nv12 || p010 || mono || yuy2 || uyvy || y210 || ppm || out_rgba8 || out_nv12 || srgb || show_mag ||
                 show_phase || ring_local > 0 || ring_world > 0)) {
        fprintf(stderr, "--i420 does not go with --nv12, --p010, --mono, --yuy2, --uyvy, --y210, --ppm, --out-rgba8, "
                        "--out-nv12, --srgb, the debug views or the ring modes\n");
        return 2;
    }
    if (i420 && !in_path) {
        fprintf(stderr, "--i420 needs an input (-i): an 8-bit 4:2:0 .y4m (C420) or raw I420 frames\n");
        return 2;
    }
    FILE *fi = in_path ? fopen(in_path, "rb") : NULL;
    const int planes3 = i420 || i010;   /* the file's frames go as they lie; the output opens after the refusals */
    FILE *fo = out_path && !planes3 ? fopen(out_path, "wb") : NULL;
    if ((in_path && !fi) || (out_path && !fo && !planes3)) { fprintf(stderr, "cannot open file\n"); return 1; }
    const int y4m_in = in_path && ends_with(in_path, ".y4m");
    const int y4m_out = out_path && ends_with(out_path, ".y4m");
    y4m_info yi = {0};
    yi.fps_num = 25;
    yi.fps_den = 1;
    int depth = 8;
    if (y4m_in) {
        if (y4m_read_header_ext(fi, &yi, &depth)) { fprintf(stderr, "%s: unsupported Y4M\n", in_path); return 1; }
        W = yi.width;
        H = yi.height;
    }
    /* --i420: the frames of a C420 .y4m are MM_I420 frames as they lie (the
     * output file is opened after the refusals: they write nothing) */
    if (i420) {
        if (y4m_in && (yi.chroma != Y4M_420 || depth != 8)) {
            fprintf(stderr, "--i420 needs an 8-bit 4:2:0 .y4m input (C420; a C420p10 stream takes --p010), "
                            "or raw I420 frames under any other extension\n");
            return 2;
        }
        if ((W | H) & 1) {
            fprintf(stderr, "--i420 needs even width and height (%dx%d)\n", W, H);
            return 2;
        }
        if (matrix_arg && strcmp(matrix_arg, "601") && strcmp(matrix_arg, "709") && strcmp(matrix_arg, "2020")) {
            fprintf(stderr, "--matrix takes 601, 709 or 2020, not %s (--i420)\n", matrix_arg);
            return 2;
        }
        g_fmt = full_range ? MM_I420_FULL : MM_I420;
        if (out_path && !(fo = fopen(out_path, "wb"))) { fprintf(stderr, "cannot open file\n"); return 1; }
    }
    /* --i010: the frames of a C420p10 .y4m are MM_I010 frames as they lie */
    if (i010) {
        if (y4m_in && (yi.chroma != Y4M_420 || depth != 10)) {
            fprintf(stderr, "--i010 needs a 10-bit 4:2:0 .y4m input (C420p10; an 8-bit C420 stream takes --i420), "
                            "or raw I010 frames under any other extension\n");
            return 2;
        }
        if ((W | H) & 1) {
            fprintf(stderr, "--i010 needs even width and height (%dx%d)\n", W, H);
            return 2;
        }
        if (matrix_arg && strcmp(matrix_arg, "601") && strcmp(matrix_arg, "709") && strcmp(matrix_arg, "2020")) {
            fprintf(stderr, "--matrix takes 601, 709 or 2020, not %s (--i010)\n", matrix_arg);
            return 2;
        }
        g_fmt = full_range ? MM_I010_FULL : MM_I010;
        if (out_path && !(fo = fopen(out_path, "wb"))) { fprintf(stderr, "cannot open file\n"); return 1; }
    }
    /* different formats in and out (mm_process_stream_convert) */
    if (out_rgba8 && out_nv12) {
        fprintf(stderr, "--out-rgba8 does not go with --out-nv12\n");
        return 2;
    }
    if (out_rgba8 && !nv12 && !p010) {
        fprintf(stderr, "--out-rgba8 needs --nv12 or --p010 (the default path's output is RGBA8 already)\n");
        return 2;
    }
    if (out_nv12) {
        if (nv12 || p010 || mono || yuy2 || uyvy || y210 || ppm || srgb || show_mag || show_phase || ring_local > 0 ||
            ring_world > 0) {
            fprintf(stderr, "--out-nv12 takes the RGBA8 input path: not with --nv12, --p010, --mono, --yuy2, --uyvy, "
                            "--y210, --ppm, --srgb, the debug views or the ring modes\n");
            return 2;
        }
        if ((W | H) & 1) {
            fprintf(stderr, "--out-nv12 needs even width and height (%dx%d)\n", W, H);
            return 2;
        }
    }
    /* --ppm: a stream of binary PPM images is a stream of MM_RGB24 frames */
    ppm_info pi = {0, 0};
    int ppm_pending = 0;   /* the first image's header is read, its pixels are not */
    if (bgr && !ppm) {
        fprintf(stderr, "--bgr needs --ppm\n");
        return 2;
    }
    if (ppm) {
        if (nv12 || p010 || mono || yuy2 || uyvy || y210 || srgb || matrix_arg || full_range || show_mag || show_phase ||
            ring_local > 0 || ring_world > 0) {
            fprintf(stderr, "--ppm does not go with --nv12, --p010, --mono, --yuy2, --uyvy, --y210, --srgb, --matrix, "
                            "--full-range, the debug views or the ring modes\n");
            return 2;
        }
        if (!fi || y4m_in || y4m_out) {
            fprintf(stderr, "--ppm needs a binary PPM stream as input (-i, P6, maxval 255) and writes one (-o)\n");
            return 2;
        }
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
        g_fmt = bgr ? MM_BGR24 : MM_RGB24;
    }
    const int p422 = yuy2 || uyvy;   /* packed 4:2:2 */
    if (y210) {   /* its 10-bit form */
        if (p422 || nv12 || p010 || mono || srgb || show_mag || show_phase || ring_local > 0 || ring_world > 0) {
            fprintf(stderr, "--y210 does not go with --yuy2, --uyvy, --nv12, --p010, --mono, --srgb, the debug views "
                            "or the ring modes\n");
            return 2;
        }
        if (!y4m_in || yi.chroma != Y4M_422 || depth != 10) {
            fprintf(stderr, "--y210 needs a 10-bit 4:2:2 .y4m input (-i, C422p10)\n");
            return 2;
        }
        if ((W | H) & 1) {
            fprintf(stderr, "--y210 needs even width and height (%dx%d)\n", W, H);
            return 2;
        }
        g_fmt = full_range ? MM_Y210_FULL : MM_Y210;
    } else if (y4m_in && yi.chroma == Y4M_422 && depth == 10) {
        fprintf(stderr, "%s is a 10-bit 4:2:2 stream (C422p10): it needs --y210 "
                        "(there is no 4:2:2 to RGBA conversion on the host)\n", in_path);
        return 2;
    } else if (p422) {
        const char *opt = yuy2 ? "--yuy2" : "--uyvy";
        if (yuy2 && uyvy) {
            fprintf(stderr, "--yuy2 does not go with --uyvy (one byte order)\n");
            return 2;
        }
        if (srgb || show_mag || show_phase || ring_local > 0 || ring_world > 0 || nv12 || p010 || mono) {
            fprintf(stderr, "%s does not go with --srgb, the debug views, the ring modes, --nv12, --p010 or --mono\n",
                    opt);
            return 2;
        }
        if (!y4m_in || yi.chroma != Y4M_422) {
            fprintf(stderr, "%s needs an 8-bit 4:2:2 .y4m input (-i, C422)\n", opt);
            return 2;
        }
        if ((W | H) & 1) {
            fprintf(stderr, "%s needs even width and height (%dx%d)\n", opt, W, H);
            return 2;
        }
        g_fmt = uyvy ? (full_range ? MM_UYVY_FULL : MM_UYVY) : (full_range ? MM_YUY2_FULL : MM_YUY2);
    } else if (y4m_in && yi.chroma == Y4M_422) {
        fprintf(stderr, "%s is a 4:2:2 stream (C422): it needs --yuy2 or --uyvy "
                        "(there is no 4:2:2 to RGBA conversion on the host)\n", in_path);
        return 2;
    }
    if (mono) {
        if (nv12 || p010 || srgb || matrix_arg || full_range) {
            fprintf(stderr, "--mono does not go with --nv12, --p010, --srgb, --matrix or --full-range\n");
            return 2;
        }
        if (ring_local > 0 || ring_world > 0) {
            fprintf(stderr, "--mono does not go with the ring modes (they take RGBA frames)\n");
            return 2;
        }
        if (!y4m_in || yi.chroma != Y4M_MONO) {
            fprintf(stderr, "--mono needs a mono .y4m input (-i, Cmono / Cmono10 / Cmono12 / Cmono16)\n");
            return 2;
        }
        g_fmt = depth == 8 ? MM_Y8 : depth == 10 ? MM_Y10 : depth == 12 ? MM_Y12 : MM_Y16;
    }
    if (p010) {
        if (nv12) {
            fprintf(stderr, "--p010 does not go with --nv12\n");
            return 2;
        }
        if (srgb || show_mag || show_phase || ring_local > 0 || ring_world > 0) {
            fprintf(stderr, "--p010 does not go with --srgb, the debug views or the ring modes\n");
            return 2;
        }
        if (!y4m_in || yi.chroma != Y4M_420) {
            fprintf(stderr, "--p010 needs a 10-bit 4:2:0 .y4m input (-i, C420p10)\n");
            return 2;
        }
        if (depth != 10) {
            fprintf(stderr, "--p010 needs a 10-bit input (C420p10); %s is 8-bit (--nv12 takes it as it is)\n",
                    in_path);
            return 2;
        }
        if ((W | H) & 1) {
            fprintf(stderr, "--p010 needs even width and height (%dx%d)\n", W, H);
            return 2;
        }
        g_fmt = full_range ? MM_P010_FULL : MM_P010;
    } else if (depth != 8 && !mono && !y210 && !i010) {
        if (yi.chroma == Y4M_MONO)
            fprintf(stderr, "%s is a %d-bit mono stream (Cmono%d): it needs --mono\n", in_path, depth, depth);
        else
            fprintf(stderr, "%s is a 10-bit stream (C420p10): it needs --p010\n", in_path);
        return 2;
    }
    if (nv12) {
        if (srgb || show_mag || show_phase || ring_local > 0 || ring_world > 0) {
            fprintf(stderr, "--nv12 does not go with --srgb, the debug views or the ring modes\n");
            return 2;
        }
        if (!y4m_in || yi.chroma != Y4M_420) {
            fprintf(stderr, "--nv12 needs a 4:2:0 .y4m input (-i)\n");
            return 2;
        }
        if ((W | H) & 1) {
            fprintf(stderr, "--nv12 needs even width and height (%dx%d)\n", W, H);
            return 2;
        }
        g_fmt = full_range ? MM_NV12_FULL : MM_NV12;
    }
    /* the output side's format: the input's, but with --out-rgba8 / --out-nv12 */
    int o_fmt = out_nv12 ? (full_range ? MM_NV12_FULL : MM_NV12) : 0;
    if (matrix_arg) {
        if (!nv12 && !p010 && !p422 && !y210 && !out_nv12 && !planes3) {
            fprintf(stderr, "--matrix needs --nv12, --p010, --yuy2, --uyvy, --y210, --i420, --i010 or --out-nv12 (the RGBA conversion of a .y4m is BT.601)\n");
            return 2;
        }
        /* (--out-nv12: the bit names the output code; the input is RGBA8) */
        int *mf = out_nv12 ? &o_fmt : &g_fmt;
        if (!strcmp(matrix_arg, "709")) *mf |= MM_MATRIX_BT709;
        else if (!strcmp(matrix_arg, "2020")) *mf |= MM_MATRIX_BT2020;
        else if (strcmp(matrix_arg, "601")) {
            fprintf(stderr, "--matrix takes 601, 709 or 2020, not %s\n", matrix_arg);
            return 2;
        }
    }
    if (out_rgba8) o_fmt = MM_RGBA8;
    else if (!out_nv12) o_fmt = g_fmt;
    const int convert = o_fmt != g_fmt;
    /* what the output files hold */
    /* (--i420: a C420 file too, its frames written as they lie) */
    /* (--i010: a C420p10 file, the same way) */
    const int w_nv12 = out_nv12 || (nv12 && !out_rgba8) || i420, w_p010 = (p010 && !out_rgba8) || i010;
    mm_params p;
    mm_params_default(&p);
    p.levels = L;
    p.phase_scale = S;
    p.mode = standard ? MM_MODE_STANDARD : orientations > 1 ? MM_MODE_STEERABLE : MM_MODE_PYRAMID;
    p.orientations = orientations;
    p.temporal_filter = iir ? MM_FILTER_IIR : MM_FILTER_DIFF;
    p.show_magnitude = show_mag;
    p.show_phase = show_phase;
    if (surf_arg && (ring_local > 0 || ring_world > 0)) {
        fprintf(stderr, "--surface-align does not go with the ring modes (they take tight frames)\n");
        return 2;
    }
    if (ring_local > 0) {
        if (fi || fo) {
            fprintf(stderr, "--ring-local needs a synthetic stream\n");
            return 2;
        }
        return run_ring_local(&p, W, H, F, B, dev, ring_local, checksum, halo, compare);
    }
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
    if (ring_world > 0) {
        if (!ring_id_path || fi || fo) {
            fprintf(stderr, "--ring-world needs --ring-id and a synthetic stream\n");
            return 2;
        }
        CHECK(mm_set_batch(h, B));
        const int rc = run_ring(h, W, H, F, B, dev, ring_world, ring_rank, ring_id_path, checksum, halo);
        mm_destroy(h);
        return rc;
    }

    size_t fb = (size_t)W * H * 4;
    if (nv12 || p010 || mono || p422 || y210 || ppm || planes3) CHECK(mm_frame_bytes(W, H, g_fmt, &fb));
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
                            "(pixel size; NV12 2, P010 and 4:2:2 4, Y210 8, mono: the sample size, --ppm and --i420: 1, --i010: 2; --i420: an even pitch, --i010: a multiple of 4) and R >= 1 (4:2:0: even)\n", surf_arg);
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
    hipStream_t s = (hipStream_t)mm_stream(h);
    unsigned char *host = (fi || fo) ? (unsigned char *)malloc((fb > fbo ? fb : fbo) * B) : NULL;
    unsigned char *planes = (y4m_in || y4m_out)
        ? (unsigned char *)malloc(y4m_in ? (y4m_frame_bytes_depth(&yi, depth) > 3 * (size_t)W * H
                                               ? y4m_frame_bytes_depth(&yi, depth) : 3 * (size_t)W * H)
                                         : 3 * (size_t)W * H)
        : NULL;
    /* (planes: 3 W H bytes hold a C420p10 frame, 2 bytes per sample, exactly; a
     * C422p10 frame takes 4 W H) */
    if (y4m_out && (mono   ? y4m_write_header_mono(fo, W, H, yi.fps_num, yi.fps_den, depth)
                    : w_p010 ? y4m_write_header_420p10(fo, W, H, yi.fps_num, yi.fps_den)
                    : w_nv12 ? y4m_write_header_420(fo, W, H, yi.fps_num, yi.fps_den)
                    : p422 ? y4m_write_header_422(fo, W, H, yi.fps_num, yi.fps_den)
                    : y210 ? y4m_write_header_422p10(fo, W, H, yi.fps_num, yi.fps_den)
                           : y4m_write_header(fo, W, H, yi.fps_num, yi.fps_den))) {
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
        if (fi && y4m_in) {
            int got = 0;
            for (; got < n; ++got) {
                /* (mono: the samples are the frame, read straight into place;
                 * --i420: the three planes are the frame, the same way) */
                const int r = mono ? y4m_read_frame_mono(fi, W, H, depth, host + fb * got)
                              : planes3 ? y4m_read_frame_depth(fi, &yi, depth, host + fb * got)
                                     : y4m_read_frame_depth(fi, &yi, depth, planes);
                if (r < 0) { fprintf(stderr, "%s: malformed frame\n", in_path); return 1; }
                if (r == 0) break;
                if (mono || planes3) continue;
                if (p010) y4m_420p10_to_p010(W, H, (const uint16_t *)planes, (uint16_t *)(host + fb * got));
                else if (nv12) y4m_420_to_nv12(W, H, planes, host + fb * got);
                else if (p422) y4m_422_to_packed(W, H, planes, host + fb * got, uyvy);
                else if (y210) y4m_422p10_to_y210(W, H, (const uint16_t *)planes, (uint16_t *)(host + fb * got));
                /* (--out-nv12: --full-range names the output code, the input is limited range) */
                else y4m_to_rgba(&yi, planes, host + fb * got, out_nv12 ? 0 : full_range);
            }
            if (got == 0) break;
            n = got;
            if (surf_copy(d_in, &lay, host, &tight, W, H, n, hipMemcpyHostToDevice, s)) return 1;
        } else if (fi && ppm) {
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
            }
            if (got == 0) break;
            n = got;
            if (surf_copy(d_in, &lay, host, &tight, W, H, n, hipMemcpyHostToDevice, s)) return 1;
        } else if (fi) {
            size_t got = fread(host, fb, (size_t)n, fi);
            if (got == 0) break;
            n = (int)got;
            if (surf_copy(d_in, &lay, host, &tight, W, H, n, hipMemcpyHostToDevice, s)) return 1;
        } else {
            CHECK(mm_synth_frames(surf_arg ? d_tin : d_in, W, H, done, n, 0x5EED0000ull, 0, s));
            if (surf_arg && surf_copy(d_in, &lay, d_tin, &tight, W, H, n, hipMemcpyDeviceToDevice, s)) return 1;
        }
        hipEventRecord(e0, s);
        if (convert) CHECK(mm_process_stream_convert(h, d_in, &lay, d_out, &olay, n, s));
        else if (surf_arg) CHECK(mm_process_stream_surfaces(h, d_in, &lay, d_out, &lay, n, s));
        else CHECK(mm_process_stream(h, d_in, d_out, n, g_fmt, s));
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
            if (y4m_out) {
                for (int k = 0; k < n; ++k) {
                    if (mono) {
                        if (y4m_write_frame_mono(fo, W, H, depth, host + fb * k)) {
                            fprintf(stderr, "write failed\n");
                            return 1;
                        }
                        continue;
                    }
                    if (i420) {   /* the frame is the file's three planes */
                        if (y4m_write_frame_420(fo, W, H, host + fb * k)) {
                            fprintf(stderr, "write failed\n");
                            return 1;
                        }
                        continue;
                    }
                    if (i010) {   /* ... its three planes of words */
                        if (y4m_write_frame_420p10(fo, W, H, (const uint16_t *)(host + fb * k))) {
                            fprintf(stderr, "write failed\n");
                            return 1;
                        }
                        continue;
                    }
                    if (w_p010) y4m_p010_to_420p10(W, H, (const uint16_t *)(host + fb * k), (uint16_t *)planes);
                    else if (w_nv12) y4m_nv12_to_420(W, H, host + fbo * k, planes);
                    else if (p422) y4m_packed_to_422(W, H, host + fb * k, planes, uyvy);
                    else if (y210) y4m_y210_to_422p10(W, H, (const uint16_t *)(host + fb * k), (uint16_t *)planes);
                    else y4m_from_rgba(W, H, host + fbo * k, planes, full_range);
                    if (w_p010   ? y4m_write_frame_420p10(fo, W, H, (const uint16_t *)planes)
                        : w_nv12 ? y4m_write_frame_420(fo, W, H, planes)
                        : p422 ? y4m_write_frame_422(fo, W, H, planes)
                        : y210 ? y4m_write_frame_422p10(fo, W, H, (const uint16_t *)planes)
                               : y4m_write_frame(fo, W, H, planes)) {
                        fprintf(stderr, "write failed\n");
                        return 1;
                    }
                }
            } else if (ppm) {   /* the same container back */
                for (int k = 0; k < n; ++k) {
                    if (bgr) ppm_swap_rb(host + fb * k, (size_t)W * H);
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
    free(planes);
    hipFree(d_in);
    hipFree(d_out);
    hipFree(d_tin);
    hipFree(d_tout);
    mm_destroy(h);
    return 0;
}
