/* host/v210.c under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone
 * program (tests/test_v210_host.py builds and runs it).  Every buffer is
 * allocated at exactly the bytes the header promises are touched, so a read or
 * write past a row's used dwords or past the last row is a finding:
 *   - the pinned vector of include/mm.h;
 *   - sizes for W % 6 in {0, 2, 4};
 *   - round trips Y210 <-> v210 and C422p10 <-> v210 at the standard pitch, at
 *     the tightest pitch (4 D(W)) and at an odd byte base, with poisoned padding
 *     that must stay as it is;
 *   - the refusals. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "v210.h"

#define CHECK(c) do { if (!(c)) { printf("san_v210: FAILED %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

static uint32_t rnd_state = 0x2100210u;
static uint32_t rnd(void)
{
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return rnd_state >> 8;
}

/* the extent of a frame: pitch (H - 1) + row bytes, not pitch H */
static size_t extent(int W, int H, size_t pitch) { return pitch * (size_t)(H - 1) + v210_row_bytes(W); }

static int round_trip(int W, int H, size_t pitch, size_t base)
{
    const size_t rb = v210_row_bytes(W), ext = extent(W, H, pitch);
    const size_t yp = 4 * (size_t)W;
    uint16_t *y210 = malloc(yp * H), *back = malloc(yp * H);
    uint16_t *planes = malloc(4 * (size_t)W * H), *pback = malloc(4 * (size_t)W * H);
    uint8_t *v = malloc(base + ext), *v2 = malloc(base + ext);
    CHECK(y210 && back && planes && pback && v && v2);
    for (size_t i = 0; i < 2 * (size_t)W * H; ++i) {
        y210[i] = (uint16_t)((rnd() & 1023u) << 6);
        planes[i] = (uint16_t)(rnd() & 1023u);
    }
    /* the code range's ends */
    y210[0] = 0, y210[1] = 1023 << 6, planes[0] = 0, planes[1] = 1023;
    memset(v, 0xA5, base + ext);
    memset(v2, 0x5A, base + ext);
    CHECK(v210_pack_y210(W, H, y210, yp, v + base, pitch) == 0);
    CHECK(v210_unpack_y210(W, H, v + base, pitch, back, yp) == 0);
    CHECK(memcmp(y210, back, yp * H) == 0);
    CHECK(v210_pack_422p10(W, H, planes, v2 + base, pitch) == 0);
    CHECK(v210_unpack_422p10(W, H, v2 + base, pitch, pback) == 0);
    CHECK(memcmp(planes, pback, 4 * (size_t)W * H) == 0);
    /* padding untouched, bits 30-31 zero */
    for (size_t i = 0; i < base; ++i) CHECK(v[i] == 0xA5 && v2[i] == 0x5A);
    for (int r = 0; r < H; ++r) {
        const size_t end = r + 1 < H ? pitch : rb;
        for (size_t i = rb; i < end; ++i)
            CHECK(v[base + r * pitch + i] == 0xA5 && v2[base + r * pitch + i] == 0x5A);
        for (size_t d = 0; d < rb / 4; ++d) CHECK(!(v[base + r * pitch + 4 * d + 3] & 0xC0));
    }
    /* low bits of a Y210 word are dropped, high bits of a C422p10 word too */
    y210[2] |= 63;
    planes[2] |= 0xFC00;
    CHECK(v210_pack_y210(W, H, y210, yp, v + base, pitch) == 0);
    CHECK(v210_unpack_y210(W, H, v + base, pitch, back, yp) == 0);
    CHECK(back[2] == (y210[2] & 0xFFC0));
    CHECK(v210_pack_422p10(W, H, planes, v2 + base, pitch) == 0);
    CHECK(v210_unpack_422p10(W, H, v2 + base, pitch, pback) == 0);
    CHECK(pback[2] == (planes[2] & 1023));
    free(y210), free(back), free(planes), free(pback), free(v), free(v2);
    return 0;
}

int main(void)
{
    /* sizes */
    CHECK(v210_row_bytes(1920) == 5120 && v210_row_bytes(1280) == 3416 && v210_row_bytes(200) == 536);
    CHECK(v210_row_bytes(98) == 264 && v210_row_bytes(64) == 172 && v210_row_bytes(6) == 16);
    CHECK(v210_row_bytes(2) == 8 && v210_row_bytes(4) == 12 && v210_row_bytes(3) == 0 && v210_row_bytes(0) == 0);
    CHECK(v210_pitch(1920) == 5120 && v210_pitch(1280) == 3456 && v210_pitch(98) == 384 && v210_pitch(64) == 256);
    CHECK(v210_pitch(48) == 128 && v210_pitch(50) == 256 && v210_pitch(0) == 0);
    /* the pinned vector: Cb Y Cr Y ... = 1 .. 12 */
    {
        const uint16_t planes[12] = {2, 4, 6, 8, 10, 12, /* Cb */ 1, 5, 9, /* Cr */ 3, 7, 11};
        const uint32_t want[4] = {0x00300801u, 0x00601404u, 0x00902007u, 0x00C02C0Au};
        uint32_t got[4];
        CHECK(v210_pack_422p10(6, 1, planes, got, 16) == 0);
        CHECK(memcmp(got, want, 16) == 0);
        uint16_t y210[12];
        CHECK(v210_unpack_y210(6, 1, want, 16, y210, 24) == 0);
        const uint16_t seq[12] = {2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11};   /* words Y0 Cb Y1 Cr */
        for (int i = 0; i < 12; ++i) CHECK(y210[i] == seq[i] << 6);
        /* bits 30-31 are ignored on input */
        uint32_t stray[4];
        for (int i = 0; i < 4; ++i) stray[i] = want[i] | 0xC0000000u;
        uint16_t y2[12];
        CHECK(v210_unpack_y210(6, 1, stray, 16, y2, 24) == 0);
        CHECK(memcmp(y210, y2, sizeof y2) == 0);
    }
    /* round trips: W % 6 = 0, 2, 4 */
    static const int sizes[][2] = {{48, 4}, {6, 2}, {98, 6}, {64, 4}, {2, 2}, {4, 2}, {200, 2}};
    for (size_t k = 0; k < sizeof sizes / sizeof *sizes; ++k) {
        const int W = sizes[k][0], H = sizes[k][1];
        if (round_trip(W, H, v210_pitch(W), 0)) return 1;
        if (round_trip(W, H, v210_row_bytes(W), 0)) return 1;   /* rows back to back */
        if (round_trip(W, H, v210_pitch(W) + 16, 3)) return 1;  /* an odd byte base: no alignment is asked */
    }
    /* refusals */
    {
        uint32_t v[8] = {0};
        uint16_t w[32] = {0};
        CHECK(v210_pack_y210(5, 2, w, 20, v, 16) == -1);          /* odd width */
        CHECK(v210_pack_y210(0, 2, w, 20, v, 16) == -1);
        CHECK(v210_pack_y210(6, 0, w, 24, v, 16) == -1);
        CHECK(v210_pack_y210(6, 1, w, 24, v, 12) == -1);          /* pitch 4 D(W) - 4 */
        CHECK(v210_pack_y210(6, 1, w, 20, v, 16) == -1);          /* Y210 pitch below 4 W */
        CHECK(v210_pack_y210(6, 1, NULL, 24, v, 16) == -1);
        CHECK(v210_unpack_y210(6, 1, v, 12, w, 24) == -1);
        CHECK(v210_pack_422p10(6, 1, w, v, 12) == -1);
        CHECK(v210_unpack_422p10(6, 1, v, 12, w) == -1);
        CHECK(v210_unpack_422p10(6, 1, NULL, 16, w) == -1);
    }
    printf("san_v210: ok\n");
    return 0;
}
