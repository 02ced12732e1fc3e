/* ppm.h — binary PPM (P6, maxval 255) frame streams for mm_cli --ppm.
 *
 * A stream is concatenated P6 images of one size, what
 *   ffmpeg -i clip -f image2pipe -vcodec ppm out.ppm
 * writes and `ffmpeg -f image2pipe -vcodec ppm -i out.ppm` reads back.  One
 * image is the header "P6 <width> <height> <maxval>" (decimal, separated by
 * any whitespace; a '#' starts a comment that runs to the end of its line),
 * ONE whitespace byte, then height rows of width pixels, bytes R G B: an
 * MM_RGB24 frame as it lies.  No colour arithmetic runs on the host; mm_cli
 * --bgr swaps R and B on read and write and sends MM_BGR24.
 *
 * Every function returns PPM_OK, PPM_EOF (a clean end of the stream: no byte
 * where the next image would start) or one negative code per cause; nothing
 * crashes on a malformed file.  Host code only: no GPU, no HIP (the CPU tests
 * load lib/libppm.so with ctypes). */
#ifndef MM_PPM_H
#define MM_PPM_H
#include <stddef.h>
#include <stdio.h>

#define PPM_OK             0
#define PPM_EOF            1   /* end of the stream in front of an image */
#define PPM_ERR_MAGIC     -1   /* not "P6" (P3 text, P5 gray, anything else) */
#define PPM_ERR_HEADER    -2   /* the header is malformed or ends early */
#define PPM_ERR_MAXVAL    -3   /* maxval is not 255 (16-bit PPM: out of scope) */
#define PPM_ERR_TRUNCATED -4   /* fewer than 3 W H pixel bytes */
#define PPM_ERR_SIZE      -5   /* an image whose size differs from the first's */
#define PPM_ERR_ARG       -6   /* a null argument */

#define PPM_MAX_DIM 65536      /* larger widths or heights: PPM_ERR_HEADER */

typedef struct {
    int width, height;
} ppm_info;

/* Reads one image's header; the stream then stands at its first pixel byte. */
int ppm_read_header(FILE *f, ppm_info *pi);
/* Reads the 3 W H pixel bytes of the image whose header was just read. */
int ppm_read_pixels(FILE *f, const ppm_info *pi, unsigned char *rgb);
/* The next image of a stream whose images are all `first`'s size: header
 * (PPM_EOF at a clean end, PPM_ERR_SIZE for another size) and pixels. */
int ppm_read_next(FILE *f, const ppm_info *first, unsigned char *rgb);
/* Writes one image: "P6\n<W> <H>\n255\n" and the pixels. */
int ppm_write_frame(FILE *f, int width, int height, const unsigned char *rgb);
/* Swaps bytes 0 and 2 of every pixel in place (R G B <-> B G R). */
void ppm_swap_rb(unsigned char *px, size_t pixels);

#endif
