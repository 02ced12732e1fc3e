/*
 * san_ppm.c — the binary PPM module (phase-based-motion-manipulation_amd/host/
 * ppm.c) under AddressSanitizer + UndefinedBehaviorSanitizer, compiled with
 * -fsanitize=address,undefined -fno-sanitize-recover=all by
 * tests/test_ppm_sanitize.py.  Host code only; exits non-zero on any finding
 * or wrong result.
 *
 * Exercised: write -> read of a stream into exactly sized heap buffers, the
 * R / B swap on an exactly sized buffer, a truncated last frame, a frame of
 * another size, every accepted header form and every refusal, and every
 * prefix of a valid stream (each must end with a status, never a crash).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ppm.h"

static FILE *file_of(const void *data, size_t n)
{
    FILE *f = tmpfile();
    if (!f) return NULL;
    if (n && fwrite(data, 1, n, f) != n) return NULL;
    rewind(f);
    return f;
}

static int header_of(const char *text, size_t n, ppm_info *pi)
{
    FILE *f = file_of(text, n);
    if (!f) return 99;
    const int rc = ppm_read_header(f, pi);
    fclose(f);
    return rc;
}

static int roundtrip(int W, int H, int n)
{
    const size_t fb = (size_t)3 * W * H;
    unsigned char *src = malloc(fb), *dst = malloc(fb);
    FILE *f = tmpfile();
    if (!src || !dst || !f) return 1;
    for (int k = 0; k < n; ++k) {
        for (size_t i = 0; i < fb; ++i) src[i] = (unsigned char)(i * 31 + 7 * (size_t)k);
        if (ppm_write_frame(f, W, H, src)) return 1;
    }
    fputs("P6\n", f);                 /* a truncated last image: header and half the pixels */
    fprintf(f, "%d %d\n255\n", W, H);
    fwrite(src, 1, fb / 2, f);
    rewind(f);
    ppm_info first;
    if (ppm_read_header(f, &first) || first.width != W || first.height != H) return 1;
    if (ppm_read_pixels(f, &first, dst)) return 1;
    int frames = 0, rc = PPM_OK;
    while (rc == PPM_OK) {
        for (size_t i = 0; i < fb; ++i)
            if (dst[i] != (unsigned char)(i * 31 + 7 * (size_t)frames)) return 1;
        ++frames;
        rc = ppm_read_next(f, &first, dst);
    }
    fclose(f);
    if (frames != n || rc != PPM_ERR_TRUNCATED) return 1;
    /* the swap touches exactly 3 W H bytes and is its own inverse */
    memcpy(dst, src, fb);
    ppm_swap_rb(dst, (size_t)W * H);
    for (size_t p = 0; p < (size_t)W * H; ++p)
        if (dst[3 * p] != src[3 * p + 2] || dst[3 * p + 1] != src[3 * p + 1] || dst[3 * p + 2] != src[3 * p]) return 1;
    ppm_swap_rb(dst, (size_t)W * H);
    if (memcmp(dst, src, fb)) return 1;
    free(src);
    free(dst);
    return 0;
}

int main(void)
{
    int bad = 0;
    bad |= roundtrip(1, 1, 2);
    bad |= roundtrip(37, 21, 3);
    bad |= roundtrip(200, 120, 2);

    static const struct { const char *text; int rc; } heads[] = {
        {"P6\n4 3\n255\n", PPM_OK}, {"P6 4 3 255 ", PPM_OK}, {"P6\t4\r\n3\v\f255\t", PPM_OK},
        {"P6\n# c\n4 3\n255\n", PPM_OK}, {"P6\n4#w\n3\n#\n# two\n255\n", PPM_OK}, {"P6#c\n4 3 255\n", PPM_OK},
        {"P3\n4 3\n255\n", PPM_ERR_MAGIC}, {"P5\n4 3\n255\n", PPM_ERR_MAGIC}, {"P", PPM_ERR_MAGIC},
        {"P6\n4 3\n65535\n", PPM_ERR_MAXVAL}, {"P6\n4 3\n254\n", PPM_ERR_MAXVAL},
        {"P65 4 255\n", PPM_ERR_HEADER}, {"P6\n4 x\n255\n", PPM_ERR_HEADER}, {"P6\n4x3\n255\n", PPM_ERR_HEADER},
        {"P6\n0 3\n255\n", PPM_ERR_HEADER}, {"P6\n-4 3\n255\n", PPM_ERR_HEADER},
        {"P6\n99999999999999999999 3\n255\n", PPM_ERR_HEADER}, {"P6\n4 3\n", PPM_ERR_HEADER},
        {"P6\n4 3\n255", PPM_ERR_HEADER}, {"P6\n4 3\n# never ends", PPM_ERR_HEADER}, {"P6", PPM_ERR_HEADER},
        {"", PPM_EOF},
    };
    for (size_t i = 0; i < sizeof heads / sizeof heads[0]; ++i) {
        ppm_info pi = {-7, -7};
        const int rc = header_of(heads[i].text, strlen(heads[i].text), &pi);
        if (rc != heads[i].rc || (rc == PPM_OK ? pi.width != 4 || pi.height != 3 : pi.width != -7)) {
            fprintf(stderr, "header %zu: status %d, want %d\n", i, rc, heads[i].rc);
            bad = 1;
        }
    }
    /* a frame of another size, and null arguments */
    {
        unsigned char px[64] = {0};
        FILE *f = tmpfile();
        if (!f || ppm_write_frame(f, 2, 3, px) || ppm_write_frame(f, 3, 2, px)) return 1;
        rewind(f);
        ppm_info first;
        if (ppm_read_header(f, &first) || ppm_read_pixels(f, &first, px)) bad = 1;
        if (ppm_read_next(f, &first, px) != PPM_ERR_SIZE) bad = 1;
        if (ppm_read_header(NULL, &first) != PPM_ERR_ARG || ppm_read_header(f, NULL) != PPM_ERR_ARG ||
            ppm_read_pixels(f, &first, NULL) != PPM_ERR_ARG || ppm_read_next(f, NULL, px) != PPM_ERR_ARG ||
            ppm_write_frame(f, 2, 3, NULL) != PPM_ERR_ARG || ppm_write_frame(f, 0, 3, px) != PPM_ERR_ARG)
            bad = 1;
        ppm_swap_rb(NULL, 4);
        fclose(f);
    }
    /* every prefix of a valid two-image stream ends with a status */
    {
        unsigned char img[2 * (11 + 18)], px[18];
        size_t n = 0;
        for (int k = 0; k < 2; ++k) {
            memcpy(img + n, "P6\n3 2\n255\n", 11);
            n += 11;
            for (int i = 0; i < 18; ++i) img[n++] = (unsigned char)(35 + i);   /* '#' first: pixel data, not a comment */
        }
        for (size_t cut = 0; cut <= n; ++cut) {
            FILE *f = file_of(img, cut);
            if (!f) return 1;
            ppm_info first;
            int rc = ppm_read_header(f, &first), frames = 0;
            if (rc == PPM_OK) rc = ppm_read_pixels(f, &first, px);
            while (rc == PPM_OK && frames < 4) {
                ++frames;
                rc = ppm_read_next(f, &first, px);
            }
            fclose(f);
            const int want = (int)(cut / 29);
            if (frames != want || (cut % 29 == 0 ? rc != PPM_EOF : rc >= 0)) {
                fprintf(stderr, "prefix %zu: %d frames, status %d\n", cut, frames, rc);
                bad = 1;
            }
        }
    }
    if (bad) return 1;
    puts("san_ppm: ok");
    return 0;
}
