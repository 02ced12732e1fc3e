/*
 * y4m.h — YUV4MPEG2 (.y4m) stream I/O and BT.601 colour conversion for the C
 * host driver (real clips instead of synthetic streams).
 *
 * Reads 8-bit 4:2:0 (C420, C420jpeg, C420paldv, C420mpeg2), 4:4:4 (C444) and
 * mono (Cmono) streams; writes 4:4:4, or 4:2:0 for the NV12 path.  Chroma is upsampled by sample
 * replication (each 4:2:0 sample covers its 2x2 block).  Colour matrix BT.601,
 * limited range (Y 16..235, C 16..240) unless `full_range` (JPEG-style 0..255).
 * Host-side only: the frames then go through mm_process_stream as RGBA8, or,
 * 4:2:0 streams re-interleaved to NV12, as MM_NV12 without any conversion;
 * 10-bit 4:2:0 (C420p10) streams likewise as MM_P010, and mono streams of 8, 10,
 * 12 or 16 bits (Cmono, Cmono10, Cmono12, Cmono16) as MM_Y8 .. MM_Y16, and
 * 8-bit 4:2:2 (C422) streams interleaved to YUY2 / UYVY as MM_YUY2 / MM_UYVY
 * and 10-bit 4:2:2 (C422p10) streams interleaved to Y210 as MM_Y210 (the last
 * four sections).  There is no 4:2:2 to RGBA conversion.
 */
#ifndef MM355_Y4M_H
#define MM355_Y4M_H

#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { Y4M_420 = 0, Y4M_444 = 1, Y4M_MONO = 2, Y4M_422 = 3 };   /* Y4M_422: y4m_read_header_depth / _ext only */

typedef struct {
    int width, height;
    int fps_num, fps_den;   /* F tag (default 25:1) */
    int aspect_num, aspect_den;
    int chroma;             /* Y4M_420 | Y4M_444 | Y4M_MONO | Y4M_422 */
    char interlace;         /* I tag, 'p' if absent */
} y4m_info;

/* Parse the stream header.  Returns 0, or -1 (not Y4M / unsupported chroma or
 * bit depth / malformed). */
int y4m_read_header(FILE *f, y4m_info *info);

/* Bytes of one frame's planes for `info`. */
size_t y4m_frame_bytes(const y4m_info *info);

/* Read one frame ("FRAME..." line + planes) into `planes`
 * (y4m_frame_bytes bytes).  Returns 1 on a frame, 0 at end of stream, -1 on
 * a malformed frame. */
int y4m_read_frame(FILE *f, const y4m_info *info, uint8_t *planes);

/* planes -> RGBA8 (alpha 255), and RGBA8 -> 4:4:4 planes (Y, Cb, Cr). */
void y4m_to_rgba(const y4m_info *info, const uint8_t *planes, uint8_t *rgba, int full_range);
void y4m_from_rgba(int width, int height, const uint8_t *rgba, uint8_t *planes444, int full_range);

/* Write a C444 header / one C444 frame. */
int y4m_write_header(FILE *f, int width, int height, int fps_num, int fps_den);
int y4m_write_frame(FILE *f, int width, int height, const uint8_t *planes444);

/* 4:2:0 planes (Y, Cb, Cr; even width and height) <-> one NV12 frame (Y, then
 * rows of interleaved Cb, Cr pairs; width * height * 3/2 bytes either way):
 * the chroma planes are interleaved / de-interleaved, no arithmetic.  Frames
 * in this layout go through mm_process_stream as MM_NV12 / MM_NV12_FULL with
 * no colour conversion on the host. */
void y4m_420_to_nv12(int width, int height, const uint8_t *planes420, uint8_t *nv12);
void y4m_nv12_to_420(int width, int height, const uint8_t *nv12, uint8_t *planes420);

/* Write a C420 header / one C420 frame (planes Y, Cb, Cr). */
int y4m_write_header_420(FILE *f, int width, int height, int fps_num, int fps_den);
int y4m_write_frame_420(FILE *f, int width, int height, const uint8_t *planes420);

/* ---- 10-bit 4:2:0 (C420p10), for the MM_P010 path -------------------------
 * Samples are 16-bit little-endian words holding 0 .. 1023, planes Y, Cb, Cr
 * (this module reads and writes them as uint16_t: little-endian hosts).
 * y4m_read_header keeps refusing the tag; these entry points stand beside it
 * and y4m_info keeps its layout (the depth travels separately). */

/* y4m_read_header that also accepts C420p10, Cmono10 / Cmono12 / Cmono16 and
 * C422: *bit_depth is 10 for C420p10 (chroma Y4M_420), 10, 12 or 16 for the
 * mono tags (chroma Y4M_MONO), 8 for C422 (chroma Y4M_422) and for every tag
 * y4m_read_header accepts. */
int y4m_read_header_depth(FILE *f, y4m_info *info, int *bit_depth);

/* Bytes of one frame's planes at `bit_depth` (2 bytes per sample above 8), and
 * y4m_read_frame for that many bytes. */
size_t y4m_frame_bytes_depth(const y4m_info *info, int bit_depth);
int y4m_read_frame_depth(FILE *f, const y4m_info *info, int bit_depth, void *planes);

/* 10-bit 4:2:0 planes (even width and height) <-> one P010 frame (Y words,
 * then rows of interleaved Cb, Cr words; 3 * width * height bytes either way):
 * interleave / de-interleave and a shift by 6 (word = sample << 6; sample =
 * word >> 6), no other arithmetic. */
void y4m_420p10_to_p010(int width, int height, const uint16_t *planes420, uint16_t *p010);
void y4m_p010_to_420p10(int width, int height, const uint16_t *p010, uint16_t *planes420);

/* Write a C420p10 header / one C420p10 frame (planes Y, Cb, Cr). */
int y4m_write_header_420p10(FILE *f, int width, int height, int fps_num, int fps_den);
int y4m_write_frame_420p10(FILE *f, int width, int height, const uint16_t *planes420);

/* ---- mono (Cmono, Cmono10, Cmono12, Cmono16), for the MM_Y8 .. MM_Y16 path ---
 * One plane of width * height samples: bytes at bit_depth 8, else 16-bit
 * little-endian words with the code in the low bits, as ffmpeg writes gray,
 * gray10le, gray12le and gray16le.  The samples are the frame as mm_process
 * takes it: no conversion either way, every bit of a word is kept.
 * y4m_read_header_depth reads the header (chroma Y4M_MONO and the depth).
 * bit_depth other than 8, 10, 12, 16: -1 from each of these. */
int y4m_write_header_mono(FILE *f, int width, int height, int fps_num, int fps_den, int bit_depth);
/* as y4m_read_frame: 1 on a frame, 0 at end of stream, -1 on a malformed one */
int y4m_read_frame_mono(FILE *f, int width, int height, int bit_depth, void *samples);
int y4m_write_frame_mono(FILE *f, int width, int height, int bit_depth, const void *samples);

/* ---- 8-bit 4:2:2 (C422), for the MM_YUY2 / MM_UYVY path ---------------------
 * Planes Y (width x height), Cb, Cr (width / 2 x height each); even width and
 * height.  y4m_read_header_depth reads the header (chroma Y4M_422, depth 8),
 * y4m_frame_bytes and y4m_read_frame take such an info; y4m_to_rgba does not
 * (there is no 4:2:2 to RGBA conversion on the host). */

/* 4:2:2 planes <-> one packed frame of width / 2 four-byte macropixels per
 * row (2 * width * height bytes either way): bytes Y0 Cb Y1 Cr (YUY2), or
 * Cb Y0 Cr Y1 with `uyvy` non-zero.  Interleave / de-interleave only, no
 * arithmetic.  Frames in this layout go through mm_process_stream as MM_YUY2 /
 * MM_UYVY (or their _FULL and matrixed forms). */
void y4m_422_to_packed(int width, int height, const uint8_t *planes422, uint8_t *out, int uyvy);
void y4m_packed_to_422(int width, int height, const uint8_t *in, uint8_t *planes422, int uyvy);

/* Write a C422 header / one C422 frame (planes Y, Cb, Cr). */
int y4m_write_header_422(FILE *f, int width, int height, int fps_num, int fps_den);
int y4m_write_frame_422(FILE *f, int width, int height, const uint8_t *planes422);

/* ---- 10-bit 4:2:2 (C422p10), for the MM_Y210 path -----------------------------
 * Planes Y (width x height), Cb, Cr (width / 2 x height each) of little-endian
 * 16-bit words, the code in the LOW 10 bits (ffmpeg's yuv422p10le); even width
 * and height.  y4m_read_header and y4m_read_header_depth keep refusing the
 * tag; the entry point below stands beside them. */

/* y4m_read_header_depth that also accepts C422p10: chroma Y4M_422 and
 * *bit_depth 10 (C422: Y4M_422 and 8).  y4m_frame_bytes_depth and
 * y4m_read_frame_depth take such an info and depth. */
int y4m_read_header_ext(FILE *f, y4m_info *info, int *bit_depth);

/* 4:2:2 10-bit planes <-> one Y210 frame of width / 2 eight-byte macropixels
 * per row (4 * width * height bytes either way): words Y0 Cb Y1 Cr, each the
 * code << 6 (out: word >> 6).  Interleave and shift only, no arithmetic.
 * Frames in this layout go through mm_process_stream as MM_Y210 (or its _FULL
 * and matrixed forms). */
void y4m_422p10_to_y210(int width, int height, const uint16_t *planes422, uint16_t *y210);
void y4m_y210_to_422p10(int width, int height, const uint16_t *y210, uint16_t *planes422);

/* Write a C422p10 header / one C422p10 frame (planes Y, Cb, Cr). */
int y4m_write_header_422p10(FILE *f, int width, int height, int fps_num, int fps_den);
int y4m_write_frame_422p10(FILE *f, int width, int height, const uint16_t *planes422);

#ifdef __cplusplus
}
#endif
#endif
