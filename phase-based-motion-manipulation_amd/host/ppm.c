/* ppm.c — binary PPM (P6, maxval 255) frame streams (ppm.h). */
#include "ppm.h"

static int is_space(int c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f'; }

/* The next byte that is neither whitespace nor inside a comment (EOF: EOF). */
static int skip_blank(FILE *f)
{
    int c = fgetc(f);
    while (c != EOF) {
        if (c == '#') {
            while (c != EOF && c != '\n' && c != '\r') c = fgetc(f);
        } else if (!is_space(c)) {
            break;
        } else {
            c = fgetc(f);
        }
    }
    return c;
}

/* One decimal field in 0 .. PPM_MAX_DIM; *term is the byte that ended it. */
static int read_number(FILE *f, int *value, int *term)
{
    int c = skip_blank(f);
    if (c < '0' || c > '9') return PPM_ERR_HEADER;
    long v = 0;
    while (c >= '0' && c <= '9') {
        v = v * 10 + (c - '0');
        if (v > PPM_MAX_DIM) return PPM_ERR_HEADER;
        c = fgetc(f);
    }
    if (c != EOF && c != '#' && !is_space(c)) return PPM_ERR_HEADER;   /* "4x3" */
    /* (a comment may follow a number directly: leave its '#' for the next field) */
    if (c == '#' && ungetc(c, f) == EOF) return PPM_ERR_HEADER;
    *value = (int)v;
    *term = c;
    return PPM_OK;
}

int ppm_read_header(FILE *f, ppm_info *pi)
{
    if (!f || !pi) return PPM_ERR_ARG;
    const int c0 = fgetc(f);
    if (c0 == EOF) return PPM_EOF;
    const int c1 = fgetc(f);
    if (c0 != 'P' || c1 != '6') return PPM_ERR_MAGIC;
    int w, h, maxval, term;
    /* ("P6" must end: "P65 4 255" is no header) */
    const int sep = fgetc(f);
    if (sep != '#' && !is_space(sep)) return PPM_ERR_HEADER;
    if (sep == '#' && ungetc(sep, f) == EOF) return PPM_ERR_HEADER;
    int rc;
    if ((rc = read_number(f, &w, &term)) || (rc = read_number(f, &h, &term)) ||
        (rc = read_number(f, &maxval, &term)))
        return rc;
    if (w < 1 || h < 1) return PPM_ERR_HEADER;
    if (maxval != 255) return PPM_ERR_MAXVAL;
    /* exactly one whitespace byte separates maxval from the pixels */
    if (!is_space(term)) return PPM_ERR_HEADER;
    pi->width = w;
    pi->height = h;
    return PPM_OK;
}

int ppm_read_pixels(FILE *f, const ppm_info *pi, unsigned char *rgb)
{
    if (!f || !pi || !rgb) return PPM_ERR_ARG;
    const size_t n = (size_t)3 * (size_t)pi->width * (size_t)pi->height;
    return fread(rgb, 1, n, f) == n ? PPM_OK : PPM_ERR_TRUNCATED;
}

int ppm_read_next(FILE *f, const ppm_info *first, unsigned char *rgb)
{
    if (!f || !first || !rgb) return PPM_ERR_ARG;
    ppm_info pi;
    const int rc = ppm_read_header(f, &pi);
    if (rc) return rc;
    if (pi.width != first->width || pi.height != first->height) return PPM_ERR_SIZE;
    return ppm_read_pixels(f, &pi, rgb);
}

int ppm_write_frame(FILE *f, int width, int height, const unsigned char *rgb)
{
    if (!f || !rgb || width < 1 || height < 1) return PPM_ERR_ARG;
    const size_t n = (size_t)3 * (size_t)width * (size_t)height;
    if (fprintf(f, "P6\n%d %d\n255\n", width, height) < 0) return PPM_ERR_TRUNCATED;
    return fwrite(rgb, 1, n, f) == n ? PPM_OK : PPM_ERR_TRUNCATED;
}

void ppm_swap_rb(unsigned char *px, size_t pixels)
{
    if (!px) return;
    for (size_t i = 0; i < pixels; ++i) {
        const unsigned char t = px[3 * i];
        px[3 * i] = px[3 * i + 2];
        px[3 * i + 2] = t;
    }
}
