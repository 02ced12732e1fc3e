/*
 * san_422p10.c — the Y4M module's 10-bit 4:2:2 entry points (C422p10:
 * phase-based-motion-manipulation_amd/host/y4m.c) under AddressSanitizer +
 * UndefinedBehaviorSanitizer, compiled with -fsanitize=address,undefined
 * -fno-sanitize-recover=all by tests/test_y210_sanitize.py.  Host code only;
 * exits non-zero on any finding or wrong result.
 *
 * Exercised: header write -> read (y4m_read_header_ext) and frame write ->
 * read of C422p10 planes, the planes interleaved to Y210 macropixels (<< 6)
 * and back in exactly sized heap buffers (word positions checked), a truncated
 * last frame, and accepted, refused, truncated and malformed headers through
 * the three header readers.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "y4m.h"

static uint16_t sample(size_t i, int k) { return (uint16_t)((i * 29 + 7 * (size_t)k + 3) & 1023); }

static int roundtrip(int W, int H)
{
    const size_t nw = (size_t)2 * W * H, nb = 2 * nw, ny = (size_t)W * H, nc = ny / 2;
    uint16_t *src = malloc(nb), *dst = malloc(nb), *pk = malloc(nb), *back = malloc(nb);
    FILE *f = tmpfile();
    if (!src || !dst || !pk || !back || !f) return 1;
    if (y4m_write_header_422p10(f, W, H, 60, 1)) return 1;
    for (int k = 0; k < 3; ++k) {
        for (size_t i = 0; i < nw; ++i) src[i] = sample(i, k);
        if (y4m_write_frame_422p10(f, W, H, src)) return 1;
    }
    fputs("FRAME\n", f);          /* truncated last frame */
    fwrite(src, 1, nb / 2, f);
    rewind(f);
    y4m_info info;
    int depth = 0, frames = 0, r, bad = 0;
    if (y4m_read_header_ext(f, &info, &depth)) return 1;
    if (info.width != W || info.height != H || info.chroma != Y4M_422 || depth != 10 || info.fps_num != 60) return 1;
    if (y4m_frame_bytes(&info) != nb / 2 || y4m_frame_bytes_depth(&info, depth) != nb) return 1;
    while ((r = y4m_read_frame_depth(f, &info, depth, dst)) == 1) {
        for (size_t i = 0; i < nw; ++i) bad |= dst[i] != sample(i, frames);
        memset(pk, 0xA5, nb);
        y4m_422p10_to_y210(W, H, dst, pk);
        const uint16_t *Y = dst, *Cb = dst + ny, *Cr = Cb + nc;
        for (size_t m = 0; m < nc; ++m) {
            const uint16_t *q = pk + 4 * m;
            bad |= q[0] != (uint16_t)(Y[2 * m] << 6) || q[1] != (uint16_t)(Cb[m] << 6) ||
                   q[2] != (uint16_t)(Y[2 * m + 1] << 6) || q[3] != (uint16_t)(Cr[m] << 6);
        }
        memset(back, 0x5A, nb);
        y4m_y210_to_422p10(W, H, pk, back);
        bad |= memcmp(back, dst, nb) != 0;
        /* Y216 content: the low bits are dropped on the way out */
        for (size_t i = 0; i < nw; ++i) pk[i] |= (uint16_t)(i & 63);
        y4m_y210_to_422p10(W, H, pk, back);
        bad |= memcmp(back, dst, nb) != 0;
        ++frames;
    }
    fclose(f);
    free(src);
    free(dst);
    free(pk);
    free(back);
    return frames == 3 && r < 0 && !bad ? 0 : 1;
}

static int headers(void)
{
    /* {text, y4m_read_header_ext's return, chroma, depth, y4m_read_header_depth's return} */
    static const struct { const char *s; int rc, chroma, depth, rc_depth; } h[] = {
        {"YUV4MPEG2 W16 H16 C422p10\n", 0, Y4M_422, 10, -1},
        {"YUV4MPEG2 W18 H6 F60:1 Ip A1:1 C422p10 Xcap=sdi\n", 0, Y4M_422, 10, -1},
        {"YUV4MPEG2 W16 H16 C422\n", 0, Y4M_422, 8, 0},
        {"YUV4MPEG2 W16 H16 C420p10\n", 0, Y4M_420, 10, 0},
        {"YUV4MPEG2 W16 H16 Cmono12\n", 0, Y4M_MONO, 12, 0},
        {"YUV4MPEG2 W16 H16 C444\n", 0, Y4M_444, 8, 0},
        {"YUV4MPEG2 W16 H16 C422p10", -1, 0, 0, -1},          /* truncated: no end of line */
        {"YUV4MPEG2 W16 H16 C422p1", -1, 0, 0, -1},
        {"YUV4MPEG2 W16 H16 C422p1\n", -1, 0, 0, -1},
        {"YUV4MPEG2 W16 H16 C422p100\n", -1, 0, 0, -1},
        {"YUV4MPEG2 W16 H16 C422p12\n", -1, 0, 0, -1},
        {"YUV4MPEG2 W16 H16 C444p10\n", -1, 0, 0, -1},
        {"YUV4MPEG2 W0 H16 C422p10\n", -1, 0, 0, -1},
        {"YUV4MPEG2 H16 C422p10\n", -1, 0, 0, -1},
        {"YUV4MPEG2 W16 H16 C422p10 F1\n", -1, 0, 0, -1},
        {"", -1, 0, 0, -1},
    };
    for (size_t i = 0; i < sizeof h / sizeof h[0]; ++i) {
        FILE *f = tmpfile();
        if (!f) return 1;
        fputs(h[i].s, f);
        rewind(f);
        y4m_info info;
        int depth = -1;
        const int rc = y4m_read_header_ext(f, &info, &depth);
        if (rc != h[i].rc || (rc == 0 && (depth != h[i].depth || info.chroma != h[i].chroma))) {
            fprintf(stderr, "header %zu: rc %d depth %d\n", i, rc, depth);
            return 1;
        }
        if (rc == 0) {   /* accepted: a frame read on the empty body must still be safe */
            void *p = malloc(y4m_frame_bytes_depth(&info, depth));
            if (!p || y4m_read_frame_depth(f, &info, depth, p) != 0) return 1;
            free(p);
        }
        /* the earlier readers keep refusing C422p10 */
        rewind(f);
        if (y4m_read_header_depth(f, &info, &depth) != h[i].rc_depth) return 1;
        rewind(f);
        if (y4m_read_header(f, &info) != (h[i].rc == 0 && h[i].depth == 8 && h[i].chroma != Y4M_422 ? 0 : -1)) return 1;
        fclose(f);
    }
    FILE *f = tmpfile();
    y4m_info info;
    if (!f || y4m_read_header_ext(f, &info, NULL) != -1) return 1;
    fclose(f);
    return 0;
}

int main(void)
{
    int fail = 0;
    fail |= roundtrip(2, 2);
    fail |= roundtrip(34, 26);
    fail |= roundtrip(98, 2);
    fail |= headers();
    printf(fail ? "san_422p10: FAILED\n" : "san_422p10: ok\n");
    return fail;
}
