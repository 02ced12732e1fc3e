/* v210.c — see v210.h. */
#include "v210.h"

#include <string.h>

size_t v210_row_bytes(int width)
{
    static const size_t part[3] = {0, 2, 3};
    if (width < 1 || (width & 1)) return 0;
    return 4 * (4 * (size_t)(width / 6) + part[(width % 6) / 2]);
}

size_t v210_pitch(int width)
{
    if (width < 1) return 0;
    return 128 * (((size_t)width + 47) / 48);
}

static int bad(int width, int height, size_t pitch)
{
    return width < 2 || (width & 1) || height < 1 || pitch < v210_row_bytes(width);
}

/* A row is the sample sequence Cb Y Cr Y ... (2 width samples), three to a
 * dword.  Sample i of a row belongs to macropixel i / 4; i % 4 is its place in
 * Cb, Y0, Cr, Y1. */

/* Y210 words lie Y0 Cb Y1 Cr: place k of the sequence is word {1, 0, 3, 2}[k] */
static const int kY210Word[4] = {1, 0, 3, 2};

static uint16_t ld16(const uint8_t *p)
{
    uint16_t v;
    memcpy(&v, p, 2);
    return v;
}

static uint32_t ld32(const uint8_t *p)
{
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}

int v210_pack_y210(int width, int height, const void *y210, size_t y210_pitch, void *v210, size_t pitch)
{
    if (bad(width, height, pitch) || !y210 || !v210 || y210_pitch < 4 * (size_t)width) return -1;
    const size_t dwords = v210_row_bytes(width) / 4, samples = 2 * (size_t)width;
    for (int r = 0; r < height; ++r) {
        const uint8_t *src = (const uint8_t *)y210 + (size_t)r * y210_pitch;
        uint8_t *dst = (uint8_t *)v210 + (size_t)r * pitch;
        for (size_t d = 0; d < dwords; ++d) {
            uint32_t w = 0;
            for (int f = 0; f < 3; ++f) {
                const size_t i = 3 * d + f;
                if (i >= samples) break;   /* the unused fields of a partial last group: zero */
                const uint16_t word = ld16(src + 2 * (4 * (i / 4) + kY210Word[i % 4]));
                w |= (uint32_t)(word >> 6) << (10 * f);
            }
            memcpy(dst + 4 * d, &w, 4);
        }
    }
    return 0;
}

int v210_unpack_y210(int width, int height, const void *v210, size_t pitch, void *y210, size_t y210_pitch)
{
    if (bad(width, height, pitch) || !y210 || !v210 || y210_pitch < 4 * (size_t)width) return -1;
    const size_t samples = 2 * (size_t)width;
    for (int r = 0; r < height; ++r) {
        const uint8_t *src = (const uint8_t *)v210 + (size_t)r * pitch;
        uint8_t *dst = (uint8_t *)y210 + (size_t)r * y210_pitch;
        for (size_t i = 0; i < samples; ++i) {
            const uint16_t word = (uint16_t)(((ld32(src + 4 * (i / 3)) >> (10 * (i % 3))) & 1023u) << 6);
            memcpy(dst + 2 * (4 * (i / 4) + kY210Word[i % 4]), &word, 2);
        }
    }
    return 0;
}

/* the C422p10 sample at place i of row r's sequence */
static const uint16_t *p422(const uint16_t *planes, int width, int height, int r, size_t i)
{
    const size_t wh = (size_t)width * height, cw = (size_t)width / 2, m = i / 4;
    switch (i % 4) {
    case 0: return planes + wh + (size_t)r * cw + m;                  /* Cb */
    case 2: return planes + wh + cw * height + (size_t)r * cw + m;    /* Cr */
    case 1: return planes + (size_t)r * width + 2 * m;                /* Y0 */
    default: return planes + (size_t)r * width + 2 * m + 1;           /* Y1 */
    }
}

int v210_pack_422p10(int width, int height, const uint16_t *planes422, void *v210, size_t pitch)
{
    if (bad(width, height, pitch) || !planes422 || !v210) return -1;
    const size_t dwords = v210_row_bytes(width) / 4, samples = 2 * (size_t)width;
    for (int r = 0; r < height; ++r) {
        uint8_t *dst = (uint8_t *)v210 + (size_t)r * pitch;
        for (size_t d = 0; d < dwords; ++d) {
            uint32_t w = 0;
            for (int f = 0; f < 3; ++f) {
                const size_t i = 3 * d + f;
                if (i >= samples) break;
                w |= (uint32_t)(*p422(planes422, width, height, r, i) & 1023u) << (10 * f);
            }
            memcpy(dst + 4 * d, &w, 4);
        }
    }
    return 0;
}

int v210_unpack_422p10(int width, int height, const void *v210, size_t pitch, uint16_t *planes422)
{
    if (bad(width, height, pitch) || !planes422 || !v210) return -1;
    const size_t samples = 2 * (size_t)width;
    for (int r = 0; r < height; ++r) {
        const uint8_t *src = (const uint8_t *)v210 + (size_t)r * pitch;
        for (size_t i = 0; i < samples; ++i)
            *(uint16_t *)p422(planes422, width, height, r, i) =
                (uint16_t)((ld32(src + 4 * (i / 3)) >> (10 * (i % 3))) & 1023u);
    }
    return 0;
}
