/*
 * san_mono.c — the Y4M module's mono entry points (Cmono, Cmono10, Cmono12,
 * Cmono16: phase-based-motion-manipulation_amd/host/y4m.c) under
 * AddressSanitizer + UndefinedBehaviorSanitizer, compiled with
 * -fsanitize=address,undefined -fno-sanitize-recover=all by
 * tests/test_mono_sanitize.py.  Host code only; exits non-zero on any finding
 * or wrong result.
 *
 * Exercised: header write -> read and frame write -> read for 1- and 2-byte
 * samples at every depth (odd sizes), a truncated last frame, a missing FRAME
 * tag, refused depths, and truncated and malformed headers.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "y4m.h"

static int roundtrip(int bits, int W, int H)
{
    const size_t bps = bits > 8 ? 2 : 1, nb = (size_t)W * H * bps;
    uint8_t *src = malloc(nb), *dst = malloc(nb);
    FILE *f = tmpfile();
    if (!src || !dst || !f) return 1;
    if (y4m_write_header_mono(f, W, H, 120, 1, bits)) return 1;
    for (int k = 0; k < 3; ++k) {
        for (size_t i = 0; i < nb; ++i) src[i] = (uint8_t)(i * 13 + 5 * k + 1);
        if (y4m_write_frame_mono(f, W, H, bits, src)) return 1;
    }
    fputs("FRAME\n", f);          /* truncated last frame */
    fwrite(src, 1, nb / 2, f);
    rewind(f);
    y4m_info info;
    int depth = 0, frames = 0, r, bad = 0;
    if (y4m_read_header_depth(f, &info, &depth)) return 1;
    if (info.width != W || info.height != H || info.chroma != Y4M_MONO || depth != bits || info.fps_num != 120)
        return 1;
    if (y4m_frame_bytes_depth(&info, depth) != nb) return 1;
    while ((r = y4m_read_frame_mono(f, W, H, bits, dst)) == 1) {
        for (size_t i = 0; i < nb; ++i) bad |= dst[i] != (uint8_t)(i * 13 + 5 * frames + 1);
        ++frames;
    }
    fclose(f);
    free(src);
    free(dst);
    return frames == 3 && r < 0 && !bad ? 0 : 1;
}

static int bad_frames(void)
{
    uint16_t buf[16 * 16] = {0};
    FILE *f = tmpfile();
    if (!f) return 1;
    fputs("FRAMX\n", f);          /* no FRAME tag */
    fwrite(buf, 1, 7, f);
    rewind(f);
    if (y4m_read_frame_mono(f, 16, 16, 12, buf) != -1) return 1;
    fclose(f);
    f = tmpfile();
    if (!f) return 1;
    fputs("FRAME", f);            /* the tag's line never ends */
    rewind(f);
    if (y4m_read_frame_mono(f, 16, 16, 16, buf) != -1) return 1;
    rewind(f);
    if (y4m_read_frame_mono(f, 16, 16, 8, buf) != -1) return 1;
    fclose(f);
    f = tmpfile();                /* empty: end of stream */
    if (!f || y4m_read_frame_mono(f, 16, 16, 10, buf) != 0) return 1;
    /* refused depths and sizes touch nothing */
    const int depths[] = {0, 1, 9, 11, 14, 15, 17, 32, -8};
    for (size_t i = 0; i < sizeof depths / sizeof depths[0]; ++i)
        if (y4m_write_header_mono(f, 16, 16, 25, 1, depths[i]) != -1 ||
            y4m_write_frame_mono(f, 16, 16, depths[i], buf) != -1 ||
            y4m_read_frame_mono(f, 16, 16, depths[i], buf) != -1)
            return 1;
    if (y4m_write_header_mono(f, 0, 16, 25, 1, 8) != -1 || y4m_write_frame_mono(f, 16, -1, 8, buf) != -1 ||
        y4m_read_frame_mono(f, -16, 16, 16, buf) != -1)
        return 1;
    fclose(f);
    return 0;
}

static int headers(void)
{
    /* {text, expected return, expected depth} */
    static const struct { const char *s; int rc, depth; } h[] = {
        {"YUV4MPEG2 W16 H16 Cmono\n", 0, 8},
        {"YUV4MPEG2 W16 H16 Cmono10\n", 0, 10},
        {"YUV4MPEG2 W17 H15 F240:1 Cmono12 Xcam=1\n", 0, 12},
        {"YUV4MPEG2 W16 H16 Cmono16\n", 0, 16},
        {"YUV4MPEG2 W16 H16 Cmono16", -1, 0},          /* truncated: no end of line */
        {"YUV4MPEG2 W16 H16 Cmo", -1, 0},
        {"YUV4MPEG2 W16 H16 Cmono1\n", -1, 0},
        {"YUV4MPEG2 W16 H16 Cmono9\n", -1, 0},
        {"YUV4MPEG2 W16 H16 Cmono14\n", -1, 0},
        {"YUV4MPEG2 W16 H16 Cmono100\n", -1, 0},
        {"YUV4MPEG2 W16 H16 Cmono12le\n", -1, 0},
        {"YUV4MPEG2 W16 H16 Cmono-12\n", -1, 0},
        {"YUV4MPEG2 W16 H16 C\n", -1, 0},
        {"YUV4MPEG2 W0 H16 Cmono12\n", -1, 0},
        {"YUV4MPEG2 H16 Cmono10\n", -1, 0},
        {"YUV4MPEG2 W16 H16 Cmono10 F1\n", -1, 0},
        {"", -1, 0},
    };
    for (size_t i = 0; i < sizeof h / sizeof h[0]; ++i) {
        FILE *f = tmpfile();
        if (!f) return 1;
        fputs(h[i].s, f);
        rewind(f);
        y4m_info info;
        int depth = -1;
        const int rc = y4m_read_header_depth(f, &info, &depth);
        if (rc != h[i].rc || (rc == 0 && (depth != h[i].depth || info.chroma != Y4M_MONO))) {
            fprintf(stderr, "header %zu: rc %d depth %d\n", i, rc, depth);
            return 1;
        }
        if (rc == 0) {   /* accepted: a frame read on the empty body must still be safe */
            void *p = malloc(y4m_frame_bytes_depth(&info, depth));
            if (!p || y4m_read_frame_mono(f, info.width, info.height, depth, p) != 0) return 1;
            free(p);
        }
        /* the 8-bit reader refuses every deeper tag */
        rewind(f);
        if (y4m_read_header(f, &info) != (h[i].rc == 0 && h[i].depth == 8 ? 0 : -1)) return 1;
        fclose(f);
    }
    return 0;
}

int main(void)
{
    int fail = 0;
    fail |= roundtrip(8, 33, 25);
    fail |= roundtrip(10, 33, 25);
    fail |= roundtrip(12, 17, 1);
    fail |= roundtrip(16, 1, 9);
    fail |= bad_frames();
    fail |= headers();
    printf(fail ? "san_mono: FAILED\n" : "san_mono: ok\n");
    return fail;
}
