/* y4m.c — see y4m.h. */
#include "y4m.h"

#include <stdlib.h>
#include <string.h>

static int clamp255(float v)
{
    int i = (int)(v + 0.5f);
    return i < 0 ? 0 : (i > 255 ? 255 : i);
}

/* "A:B" -> a, b */
static int parse_ratio(const char *s, int *a, int *b)
{
    return sscanf(s, "%d:%d", a, b) == 2 ? 0 : -1;
}

/* depth: NULL refuses the high-bit-depth tags (y4m_read_header); p422p10:
 * C422p10 is accepted too (y4m_read_header_ext) */
static int read_header(FILE *f, y4m_info *info, int *depth, int p422p10)
{
    char line[512];
    size_t n = 0;
    int c;
    while ((c = fgetc(f)) != EOF && c != '\n')
        if (n + 1 < sizeof(line)) line[n++] = (char)c;
    if (c != '\n') return -1;
    line[n] = 0;
    if (strncmp(line, "YUV4MPEG2", 9) != 0) return -1;
    memset(info, 0, sizeof(*info));
    info->fps_num = 25;
    info->fps_den = 1;
    info->aspect_num = info->aspect_den = 1;
    info->chroma = Y4M_420;
    info->interlace = 'p';
    if (depth) *depth = 8;
    char *save = NULL;
    for (char *tok = strtok_r(line + 9, " ", &save); tok; tok = strtok_r(NULL, " ", &save)) {
        const char *v = tok + 1;
        switch (tok[0]) {
        case 'W': info->width = atoi(v); break;
        case 'H': info->height = atoi(v); break;
        case 'F': if (parse_ratio(v, &info->fps_num, &info->fps_den)) return -1; break;
        case 'A': if (parse_ratio(v, &info->aspect_num, &info->aspect_den)) return -1; break;
        case 'I': info->interlace = v[0]; break;
        case 'C':
            if (!strcmp(v, "420") || !strcmp(v, "420jpeg") || !strcmp(v, "420paldv") ||
                !strcmp(v, "420mpeg2"))
                info->chroma = Y4M_420;
            else if (depth && !strcmp(v, "420p10")) {
                info->chroma = Y4M_420;
                *depth = 10;
            } else if (!strcmp(v, "444")) info->chroma = Y4M_444;
            else if (!strcmp(v, "mono")) info->chroma = Y4M_MONO;
            else if (depth && (!strcmp(v, "mono10") || !strcmp(v, "mono12") || !strcmp(v, "mono16"))) {
                info->chroma = Y4M_MONO;
                *depth = atoi(v + 4);
            }
            else if (depth && !strcmp(v, "422")) info->chroma = Y4M_422;
            else if (depth && p422p10 && !strcmp(v, "422p10")) {
                info->chroma = Y4M_422;
                *depth = 10;
            }
            else return -1;   /* 411, other high bit depths, alpha: unsupported */
            break;
        default: break;       /* X (comments) and unknown tags */
        }
    }
    if (info->width <= 0 || info->height <= 0) return -1;
    return 0;
}

int y4m_read_header(FILE *f, y4m_info *info)
{
    return read_header(f, info, NULL, 0);
}

int y4m_read_header_depth(FILE *f, y4m_info *info, int *bit_depth)
{
    return bit_depth ? read_header(f, info, bit_depth, 0) : -1;
}

int y4m_read_header_ext(FILE *f, y4m_info *info, int *bit_depth)
{
    return bit_depth ? read_header(f, info, bit_depth, 1) : -1;
}

size_t y4m_frame_bytes(const y4m_info *info)
{
    const size_t w = (size_t)info->width, h = (size_t)info->height;
    if (info->chroma == Y4M_MONO) return w * h;
    if (info->chroma == Y4M_444) return 3 * w * h;
    if (info->chroma == Y4M_422) return w * h + 2 * ((w + 1) / 2) * h;
    const size_t cw = (w + 1) / 2, ch = (h + 1) / 2;
    return w * h + 2 * cw * ch;
}

size_t y4m_frame_bytes_depth(const y4m_info *info, int bit_depth)
{
    return y4m_frame_bytes(info) * (bit_depth > 8 ? 2 : 1);
}

static int read_frame(FILE *f, size_t nb, void *planes)
{
    char tag[6];
    if (fread(tag, 1, 5, f) != 5) return 0;
    tag[5] = 0;
    if (strcmp(tag, "FRAME") != 0) return -1;
    int c;
    while ((c = fgetc(f)) != EOF && c != '\n') {}   /* frame parameters: ignored */
    if (c != '\n') return -1;
    return fread(planes, 1, nb, f) == nb ? 1 : -1;
}

int y4m_read_frame(FILE *f, const y4m_info *info, uint8_t *planes)
{
    return read_frame(f, y4m_frame_bytes(info), planes);
}

int y4m_read_frame_depth(FILE *f, const y4m_info *info, int bit_depth, void *planes)
{
    return read_frame(f, y4m_frame_bytes_depth(info, bit_depth), planes);
}

void y4m_to_rgba(const y4m_info *info, const uint8_t *planes, uint8_t *rgba, int full_range)
{
    const int W = info->width, H = info->height;
    const int cw = info->chroma == Y4M_420 ? (W + 1) / 2 : W;
    const uint8_t *Yp = planes;
    const uint8_t *Cb = planes + (size_t)W * H;
    const uint8_t *Cr = Cb + (size_t)cw * (info->chroma == Y4M_420 ? (H + 1) / 2 : H);
    /* BT.601: limited range scales Y by 255/219 and C by 255/224 */
    const float ky = full_range ? 1.0f : 255.0f / 219.0f, y0 = full_range ? 0.0f : 16.0f;
    const float kc = full_range ? 1.0f : 255.0f / 224.0f;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const float Y = ((float)Yp[(size_t)y * W + x] - y0) * ky;
            float cb = 0.0f, cr = 0.0f;
            if (info->chroma != Y4M_MONO) {
                const size_t ci = info->chroma == Y4M_420 ? (size_t)(y / 2) * cw + x / 2
                                                          : (size_t)y * W + x;
                cb = ((float)Cb[ci] - 128.0f) * kc;
                cr = ((float)Cr[ci] - 128.0f) * kc;
            }
            uint8_t *o = rgba + ((size_t)y * W + x) * 4;
            o[0] = (uint8_t)clamp255(Y + 1.402f * cr);
            o[1] = (uint8_t)clamp255(Y - 0.344136f * cb - 0.714136f * cr);
            o[2] = (uint8_t)clamp255(Y + 1.772f * cb);
            o[3] = 255;
        }
}

void y4m_from_rgba(int W, int H, const uint8_t *rgba, uint8_t *planes444, int full_range)
{
    const float ky = full_range ? 1.0f : 219.0f / 255.0f, y0 = full_range ? 0.0f : 16.0f;
    const float kc = full_range ? 1.0f : 224.0f / 255.0f;
    uint8_t *Yp = planes444, *Cb = planes444 + (size_t)W * H, *Cr = Cb + (size_t)W * H;
    for (size_t i = 0; i < (size_t)W * H; ++i) {
        const float r = rgba[4 * i], g = rgba[4 * i + 1], b = rgba[4 * i + 2];
        const float Y = 0.299f * r + 0.587f * g + 0.114f * b;
        Yp[i] = (uint8_t)clamp255(Y * ky + y0);
        Cb[i] = (uint8_t)clamp255((b - Y) * (0.5f / 0.886f) * kc + 128.0f);
        Cr[i] = (uint8_t)clamp255((r - Y) * (0.5f / 0.701f) * kc + 128.0f);
    }
}

int y4m_write_header(FILE *f, int W, int H, int fps_num, int fps_den)
{
    return fprintf(f, "YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C444\n", W, H, fps_num, fps_den) > 0 ? 0 : -1;
}

int y4m_write_frame(FILE *f, int W, int H, const uint8_t *planes444)
{
    if (fputs("FRAME\n", f) < 0) return -1;
    const size_t nb = (size_t)3 * W * H;
    return fwrite(planes444, 1, nb, f) == nb ? 0 : -1;
}

void y4m_420_to_nv12(int W, int H, const uint8_t *planes420, uint8_t *nv12)
{
    const size_t ny = (size_t)W * H, nc = ny / 4;
    const uint8_t *Cb = planes420 + ny, *Cr = Cb + nc;
    memcpy(nv12, planes420, ny);
    for (size_t i = 0; i < nc; ++i) {
        nv12[ny + 2 * i] = Cb[i];
        nv12[ny + 2 * i + 1] = Cr[i];
    }
}

void y4m_nv12_to_420(int W, int H, const uint8_t *nv12, uint8_t *planes420)
{
    const size_t ny = (size_t)W * H, nc = ny / 4;
    uint8_t *Cb = planes420 + ny, *Cr = Cb + nc;
    memcpy(planes420, nv12, ny);
    for (size_t i = 0; i < nc; ++i) {
        Cb[i] = nv12[ny + 2 * i];
        Cr[i] = nv12[ny + 2 * i + 1];
    }
}

int y4m_write_header_420(FILE *f, int W, int H, int fps_num, int fps_den)
{
    return fprintf(f, "YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C420\n", W, H, fps_num, fps_den) > 0 ? 0 : -1;
}

int y4m_write_frame_420(FILE *f, int W, int H, const uint8_t *planes420)
{
    if (fputs("FRAME\n", f) < 0) return -1;
    const size_t nb = (size_t)W * H * 3 / 2;
    return fwrite(planes420, 1, nb, f) == nb ? 0 : -1;
}

void y4m_420p10_to_p010(int W, int H, const uint16_t *planes420, uint16_t *p010)
{
    const size_t ny = (size_t)W * H, nc = ny / 4;
    const uint16_t *Cb = planes420 + ny, *Cr = Cb + nc;
    for (size_t i = 0; i < ny; ++i) p010[i] = (uint16_t)(planes420[i] << 6);
    for (size_t i = 0; i < nc; ++i) {
        p010[ny + 2 * i] = (uint16_t)(Cb[i] << 6);
        p010[ny + 2 * i + 1] = (uint16_t)(Cr[i] << 6);
    }
}

void y4m_p010_to_420p10(int W, int H, const uint16_t *p010, uint16_t *planes420)
{
    const size_t ny = (size_t)W * H, nc = ny / 4;
    uint16_t *Cb = planes420 + ny, *Cr = Cb + nc;
    for (size_t i = 0; i < ny; ++i) planes420[i] = (uint16_t)(p010[i] >> 6);
    for (size_t i = 0; i < nc; ++i) {
        Cb[i] = (uint16_t)(p010[ny + 2 * i] >> 6);
        Cr[i] = (uint16_t)(p010[ny + 2 * i + 1] >> 6);
    }
}

int y4m_write_header_420p10(FILE *f, int W, int H, int fps_num, int fps_den)
{
    return fprintf(f, "YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C420p10\n", W, H, fps_num, fps_den) > 0 ? 0 : -1;
}

int y4m_write_frame_420p10(FILE *f, int W, int H, const uint16_t *planes420)
{
    if (fputs("FRAME\n", f) < 0) return -1;
    const size_t nb = (size_t)W * H * 3;
    return fwrite(planes420, 1, nb, f) == nb ? 0 : -1;
}

static const char *mono_tag(int bit_depth)
{
    return bit_depth == 8 ? "mono" : bit_depth == 10 ? "mono10" : bit_depth == 12 ? "mono12"
           : bit_depth == 16 ? "mono16" : NULL;
}

int y4m_write_header_mono(FILE *f, int W, int H, int fps_num, int fps_den, int bit_depth)
{
    const char *tag = mono_tag(bit_depth);
    if (!tag || W <= 0 || H <= 0) return -1;
    return fprintf(f, "YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C%s\n", W, H, fps_num, fps_den, tag) > 0 ? 0 : -1;
}

int y4m_read_frame_mono(FILE *f, int W, int H, int bit_depth, void *samples)
{
    if (!mono_tag(bit_depth) || W <= 0 || H <= 0) return -1;
    return read_frame(f, (size_t)W * H * (bit_depth > 8 ? 2 : 1), samples);
}

int y4m_write_frame_mono(FILE *f, int W, int H, int bit_depth, const void *samples)
{
    if (!mono_tag(bit_depth) || W <= 0 || H <= 0) return -1;
    if (fputs("FRAME\n", f) < 0) return -1;
    const size_t nb = (size_t)W * H * (bit_depth > 8 ? 2 : 1);
    return fwrite(samples, 1, nb, f) == nb ? 0 : -1;
}

void y4m_422_to_packed(int W, int H, const uint8_t *planes422, uint8_t *out, int uyvy)
{
    const size_t ny = (size_t)W * H, nc = ny / 2;
    const uint8_t *Y = planes422, *Cb = planes422 + ny, *Cr = Cb + nc;
    const int yo = uyvy ? 1 : 0, co = uyvy ? 0 : 1;
    for (size_t i = 0; i < nc; ++i) {   /* macropixel i: pixels 2 i, 2 i + 1 (W even: never across rows) */
        uint8_t *m = out + 4 * i;
        m[yo] = Y[2 * i];
        m[yo + 2] = Y[2 * i + 1];
        m[co] = Cb[i];
        m[co + 2] = Cr[i];
    }
}

void y4m_packed_to_422(int W, int H, const uint8_t *in, uint8_t *planes422, int uyvy)
{
    const size_t ny = (size_t)W * H, nc = ny / 2;
    uint8_t *Y = planes422, *Cb = planes422 + ny, *Cr = Cb + nc;
    const int yo = uyvy ? 1 : 0, co = uyvy ? 0 : 1;
    for (size_t i = 0; i < nc; ++i) {
        const uint8_t *m = in + 4 * i;
        Y[2 * i] = m[yo];
        Y[2 * i + 1] = m[yo + 2];
        Cb[i] = m[co];
        Cr[i] = m[co + 2];
    }
}

int y4m_write_header_422(FILE *f, int W, int H, int fps_num, int fps_den)
{
    return fprintf(f, "YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C422\n", W, H, fps_num, fps_den) > 0 ? 0 : -1;
}

int y4m_write_frame_422(FILE *f, int W, int H, const uint8_t *planes422)
{
    if (fputs("FRAME\n", f) < 0) return -1;
    const size_t nb = (size_t)W * H * 2;
    return fwrite(planes422, 1, nb, f) == nb ? 0 : -1;
}

void y4m_422p10_to_y210(int W, int H, const uint16_t *planes422, uint16_t *y210)
{
    const size_t ny = (size_t)W * H, nc = ny / 2;
    const uint16_t *Y = planes422, *Cb = planes422 + ny, *Cr = Cb + nc;
    for (size_t i = 0; i < nc; ++i) {   /* macropixel i: pixels 2 i, 2 i + 1 (W even: never across rows) */
        uint16_t *m = y210 + 4 * i;
        m[0] = (uint16_t)(Y[2 * i] << 6);
        m[1] = (uint16_t)(Cb[i] << 6);
        m[2] = (uint16_t)(Y[2 * i + 1] << 6);
        m[3] = (uint16_t)(Cr[i] << 6);
    }
}

void y4m_y210_to_422p10(int W, int H, const uint16_t *y210, uint16_t *planes422)
{
    const size_t ny = (size_t)W * H, nc = ny / 2;
    uint16_t *Y = planes422, *Cb = planes422 + ny, *Cr = Cb + nc;
    for (size_t i = 0; i < nc; ++i) {
        const uint16_t *m = y210 + 4 * i;
        Y[2 * i] = (uint16_t)(m[0] >> 6);
        Cb[i] = (uint16_t)(m[1] >> 6);
        Y[2 * i + 1] = (uint16_t)(m[2] >> 6);
        Cr[i] = (uint16_t)(m[3] >> 6);
    }
}

int y4m_write_header_422p10(FILE *f, int W, int H, int fps_num, int fps_den)
{
    return fprintf(f, "YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C422p10\n", W, H, fps_num, fps_den) > 0 ? 0 : -1;
}

int y4m_write_frame_422p10(FILE *f, int W, int H, const uint16_t *planes422)
{
    if (fputs("FRAME\n", f) < 0) return -1;
    const size_t nb = (size_t)W * H * 4;
    return fwrite(planes422, 1, nb, f) == nb ? 0 : -1;
}
