/*
 * v210.h — host-side pack / unpack of v210 frames (include/mm.h, MM_V210): the
 * 10-bit 4:2:2 layout of SDI / HDMI capture cards and of ffmpeg's v210 codec.
 *
 * Each little-endian dword holds three 10-bit codes in bits 0-9, 10-19 and
 * 20-29 (bits 30-31 zero on output, ignored on input); six pixels make a group
 * of four dwords:
 *     dword 0:  Cb(0,1)  Y0       Cr(0,1)
 *     dword 1:  Y1       Cb(2,3)  Y2
 *     dword 2:  Cr(2,3)  Y3       Cb(4,5)
 *     dword 3:  Y4       Cr(4,5)  Y5
 * A row of `width` pixels (even) uses D = 4 (width / 6) + {0, 2, 3}[(width % 6)
 * / 2] dwords; the unused fields of a partial last group's dwords are written
 * as zero.  Rows lie `pitch` bytes apart; every SDK and ffmpeg use
 * v210_pitch(width) = 128 ceil(width / 48).  Bytes of a row past its 4 D are
 * padding: never read, never written.
 *
 * No arithmetic beyond shifts: a Y210 word is code << 6 (pack: word >> 6, the
 * low 6 bits dropped), a C422p10 sample is the code in the word's low 10 bits
 * (pack: sample & 1023).  Little-endian hosts (dwords and words are read and
 * written as uint32_t / uint16_t through memcpy: no alignment is asked of the
 * byte pointers).  Every function returns 0, or -1 for width < 2, an odd width,
 * height < 1 or a pitch below the row's bytes.
 */
#ifndef MM355_V210_H
#define MM355_V210_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the used dwords of one row, 4 D(width); 0 for an odd or non-positive width. */
size_t v210_row_bytes(int width);
/* The standard pitch, 128 ceil(width / 48); 0 for a non-positive width. */
size_t v210_pitch(int width);

/* Y210 frame (rows of width / 2 macropixels, words Y0 Cb Y1 Cr, y210_pitch
 * bytes apart) <-> v210 frame. */
int v210_pack_y210(int width, int height, const void *y210, size_t y210_pitch, void *v210, size_t pitch);
int v210_unpack_y210(int width, int height, const void *v210, size_t pitch, void *y210, size_t y210_pitch);

/* C422p10 planes as a .y4m frame holds them (Y width x height words, then Cb
 * and Cr, width / 2 x height words each, tight) <-> v210 frame. */
int v210_pack_422p10(int width, int height, const uint16_t *planes422, void *v210, size_t pitch);
int v210_unpack_422p10(int width, int height, const void *v210, size_t pitch, uint16_t *planes422);

#ifdef __cplusplus
}
#endif
#endif
