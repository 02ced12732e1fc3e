/*
 * mm.h — C-ABI of the MI355X-native MotionMagnificationProcessor frame operator.
 *
 * Drop-in boundary for the reference Unity component
 *   [RequireComponent(typeof(Camera))] public class MotionMagnificationProcessor
 *   (Assets/Scripts/MotionMagnificationProcessor.cs:4-5)
 * whose per-frame entry point is the image-effect callback
 *   void OnRenderImage(RenderTexture source, RenderTexture destination)  (.cs:101)
 * An RGBA frame goes in, the PhaseScale-amplified frame comes out.
 *
 * Conventions
 *   - Every function returns MM_OK (0) or a negative MM_ERR_* code; nothing
 *     throws or aborts across the ABI.  mm_strerror() names a code.
 *   - Frames are caller-owned, row-major, H rows of W RGBA pixels, tightly
 *     packed (pitch = W * bytes-per-pixel, mm_frame_bytes) or, through the
 *     mm_surface entry points, with a row pitch, a chroma-plane offset and a
 *     frame stride of the caller's.  RGBA8 is UNORM
 *     (v = byte/255); RGBA32F and RGBA16F are linear float; RGBA8_SRGB is an
 *     8-bit sRGB target as Unity's Linear colour space sees it (decoded to
 *     linear light on read, encoded on write).  MM_NV12 / MM_NV12_FULL are
 *     video frames, planar Y'CbCr 4:2:0, and MM_P010 / MM_P010_FULL their
 *     10-bit form, BT.601 or with a matrix bit BT.709 / BT.2020 (see the
 *     format list); MM_YUY2 / MM_UYVY are packed 4:2:2 capture frames and
 *     MM_Y210 / MM_Y210_FULL their 10-bit form; MM_BGRA8 / MM_BGRA8_SRGB are
 *     MM_RGBA8 / MM_RGBA8_SRGB in the byte order B G R A.  The handle
 *     owns all device scratch and the one-frame temporal state.
 *   - A handle is not thread-safe: one handle per video stream, calls in frame
 *     order (Unity calls OnRenderImage serially on its render thread).
 *   - The first frame after mm_create/mm_reset is passed through bitwise
 *     (alpha included) and becomes the temporal state (.cs:111-117); after
 *     that output alpha is 1 (CombineYIQChannels.shader:56).
 *   - Geometry: the padded square is N = nextpow2(max(W, H)) (.cs:298-302);
 *     this build covers 16 <= N <= 8192, i.e. 9 <= max(W, H) <= 8192 (other
 *     sizes: MM_ERR_UNSUPPORTED from mm_create); MM_MODE_STEERABLE stops at
 *     N = 4096.  Odd W or H are supported in every mode (and the debug
 *     views); the NV12 and P010 formats, being 4:2:0, take even W and H only and no
 *     debug view (MM_ERR_UNSUPPORTED).  The fused K3+K4 kernel runs for
 *     even sizes with W % 8 == 0 and margins N - W >= 8, N - H >= 4; every
 *     other geometry takes the unfused pair (same results).
 *   - Every entry point that takes a handle runs on the handle's device and
 *     restores the caller's current HIP device before it returns.
 */
#ifndef MM_H
#define MM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MM_ABI_VERSION 10  /* 8: the state is G_{t-1} (row spectra), see mm_state_size;
                              9: handle-scoped teardown and batch changes (mm_destroy,
                                 mm_set_batch), no device-wide synchronisation;
                             10: MM_RGBA16F and MM_RGBA8_SRGB frames, mm_frame_bytes */

/* error codes */
#define MM_OK               0
#define MM_ERR_INVALID     -1  /* bad argument / handle */
#define MM_ERR_UNSUPPORTED -2  /* geometry or mode not supported by this build */
#define MM_ERR_HIP         -3  /* HIP runtime error (launch, copy, ...) */
#define MM_ERR_NO_DEVICE   -4  /* no usable gfx950 device */
#define MM_ERR_OOM         -5  /* device allocation failed */
#define MM_ERR_NO_STATE    -6  /* mm_get_state before any frame was seen */

/* frame formats (every entry point that takes frames takes each of them;
 * the NV12 and P010 pairs for even W and H and without the debug views; the
 * single-plane grayscale formats MM_Y8 .. MM_Y16, packed 4:2:2 MM_YUY2 /
 * MM_UYVY, 10-bit packed 4:2:2 MM_Y210, packed RGB MM_RGB24 / MM_BGR24, the
 * three-plane MM_I420 / MM_I010, MM_V210 and the B G R A orders MM_BGRA8 /
 * MM_BGRA8_SRGB further down) */
#define MM_RGBA8   0       /* 4 B/px, UNORM: v = byte / 255; out round(saturate(v) * 255) */
#define MM_RGBA32F 1       /* 16 B/px, linear float                                       */
/* The frames the reference actually receives (since ABI 10): its camera
 * renders HDR (Assets/Scenes/SampleScene.unity:663, m_HDR: 1) in Linear colour
 * space (ProjectSettings/ProjectSettings.asset:50, m_ActiveColorSpace: 1), so
 * OnRenderImage's source (.cs:101) is a linear half-float target (values may
 * exceed 1) that .cs:109 blits into ARGBFloat; an LDR camera's 8-bit target is
 * sRGB, sampled as linear light and encoded on write. */
#define MM_RGBA16F    2    /* 8 B/px, linear IEEE half; values above 1 pass until the
                              reference's saturate (YIQToRGB); out rounded to nearest
                              even half, alpha 1.0                                   */
#define MM_RGBA8_SRGB 3    /* 4 B/px, sRGB-encoded bytes: in = the exact IEC 61966-2-1
                              decode of each byte (a 256-entry fp32 table), the whole
                              pipeline in linear light, out = the byte whose sRGB
                              interval holds saturate(v) (halfway points in linear
                              light; tools/gen_srgb.py); alpha byte / 255, out 255    */

/* Video frames (backward-compatible addition to ABI 10: a caller detects it by
 * mm_frame_bytes(W, H, MM_NV12, &n) == MM_OK).  8-bit Y'CbCr 4:2:0 as a
 * decoder hands it out, tightly packed: H rows of W luma bytes, then H/2 rows
 * of W bytes of interleaved (Cb, Cr) pairs, W H 3/2 bytes in all; frame k of a
 * stream at k * mm_frame_bytes; frame pointers 4-byte aligned.  W and H even (else MM_ERR_UNSUPPORTED from
 * mm_frame_bytes and every frame entry point); show_magnitude / show_phase
 * are refused with MM_ERR_UNSUPPORTED (R-channel views).
 * The frame IS the RGBA32F frame of its BT.601 decode, and the result the
 * reference's result on that frame:
 *   in:  y = (Y - 16) / 219, cb = (Cb - 128) / 224, cr = (Cr - 128) / 224
 *        (MM_NV12_FULL: Y / 255, (C - 128) / 255), every chroma sample shared
 *        by its 2 x 2 pixels; R = y + 1.402 cr, G = y - 0.344136 cb -
 *        0.714136 cr, B = y + 1.772 cb, alpha 1, NOT clamped (out-of-gamut
 *        values pass until the reference's saturate, like HDR values);
 *   out: of the saturated RGB, Yl = 0.299 R + 0.587 G + 0.114 B,
 *        Cb' = (B - Yl) 0.5 / 0.886, Cr' = (R - Yl) 0.5 / 0.701; luma code
 *        Yl 219 + 16 (full: Yl 255), chroma code 128 + 224 (full: 255) x the
 *        mean of the 2 x 2 pixels' C'; codes floor(v + 0.5) clamped to 0..255.
 * The operator changes luma only and these are RGBToYIQ's own luma weights, so
 * the kernels read the luma plane for the transform and the half-resolution
 * chroma plane for the recombination: no colour conversion on the host, 1.5
 * bytes per pixel each way.  The first frame and apply_magnification = 0 pass
 * all W H 3/2 bytes through. */
#define MM_NV12      16   /* 8-bit 4:2:0, BT.601 limited ("video") range */
#define MM_NV12_FULL 17   /* the same, full ("JPEG") range               */

/* 10-bit video frames (backward-compatible addition to ABI 10: a caller detects
 * it by mm_frame_bytes(W, H, MM_P010, &n) == MM_OK).  10-bit Y'CbCr 4:2:0 as a
 * HEVC Main10 / AV1 decoder hands it out (P010 / P016 surfaces), tightly
 * packed little-endian 16-bit words: H rows of W luma words, then H/2 rows of
 * W words of interleaved (Cb, Cr) pairs, 3 W H bytes in all; frame k of a
 * stream at k * mm_frame_bytes; frame pointers 4-byte aligned (as NV12, no
 * stricter).  W and H even (else MM_ERR_UNSUPPORTED from mm_frame_bytes and
 * every frame entry point); show_magnitude / show_phase are refused with
 * MM_ERR_UNSUPPORTED.
 * The sample is the word read as 16-bit fixed point, v = word / 64 in 10-bit
 * code units: P010 content has the low 6 bits zero; P016 content uses them and
 * they are honoured, so a P016 surface is accepted as it is.
 *   in:  y = (v - 64) / 876, cb = (v - 512) / 896, cr = (v - 512) / 896
 *        (MM_P010_FULL: v / 1023, (v - 512) / 1023); from there exactly as
 *        NV12: every chroma sample shared by its 2 x 2 pixels, the same BT.601
 *        matrix, alpha 1, NOT clamped.  Neutral chroma (word 0x8000) gives
 *        exactly zero I and Q.
 *   out: NV12's formulas on the saturated RGB; luma code Yl 876 + 64 (full:
 *        Yl 1023), chroma code 512 + 896 (full: 1023) x the mean of the 2 x 2
 *        pixels' C'; codes floor(v + 0.5) clamped to 0..1023, stored as
 *        code << 6: the low 6 bits of every output word are zero.
 * The frame IS the RGBA32F frame of that decode and the result the reference's
 * result on it; 3 bytes per pixel each way and no conversion on the host, with
 * a quarter of an 8-bit source's luma quantisation noise for phase_scale to
 * amplify.  The first frame and apply_magnification = 0 pass all 3 W H bytes
 * through bitwise, low bits included.
 * These four codes are BT.601, whose luma weights are RGBToYIQ's own (what
 * lets the transform read the luma plane alone); the matrix bits below select
 * BT.709 or BT.2020. */
#define MM_P010      18   /* 10-bit 4:2:0, BT.601 matrix, limited range */
#define MM_P010_FULL 19   /* the same, full range                        */

/* HD and UHD video frames (backward-compatible addition to ABI 10: a caller
 * detects it by mm_frame_bytes(W, H, MM_NV12 | MM_MATRIX_BT709, &n) == MM_OK).
 * One matrix bit, OR-ed onto one of the four 4:2:0 codes above, names the
 * Y'CbCr matrix of the content: H.264 / HEVC / AV1 at 720p and above is
 * BT.709, 10-bit HEVC Main10 / AV1 BT.709 or BT.2020.  The valid formats are
 * then 16..19 (BT.601, unchanged), 48..51 and 80..83 (8-bit BT.2020 included).
 * A matrix bit on an RGBA format, both bits together or any other unknown bit
 * is MM_ERR_INVALID from mm_frame_bytes, mm_surface_* and every frame entry
 * point, before anything is queued; the handle stays usable.  Layout, sizes,
 * surface units (2 and 4), even W and H, no debug views, in_layout->format ==
 * out_layout->format and the bitwise passthrough of the first frame and of
 * apply_magnification = 0 are the base code's.
 * With (Kr, Kb) the bit's and Kg = 1 - Kr - Kb, the frame IS the RGBA32F frame
 * of this decode and the result the reference's result on it:
 *   in:  y, cb, cr from the codes by the range's scales exactly as above
 *        (limited / _FULL; P010 in word units); R = y + 2 (1 - Kr) cr,
 *        B = y + 2 (1 - Kb) cb, G = y - (2 Kb (1 - Kb) / Kg) cb -
 *        (2 Kr (1 - Kr) / Kg) cr, alpha 1, NOT clamped, every chroma sample
 *        shared by its 2 x 2 pixels;
 *   out: of the saturated RGB, Y' = Kr R + Kg G + Kb B, Cb' = (B - Y') /
 *        (2 (1 - Kb)), Cr' = (R - Y') / (2 (1 - Kr)); codes, the mean of the
 *        2 x 2 pixels' C', rounding and clamps exactly as NV12 / P010 above.
 * No shortcut: Y' is not the reference's luma here.  RGBToYIQ's luma of the
 * decoded pixel is Yq = y + a cb + b cr with
 *   a = 0.114 x 2 (1 - Kb) - 0.587 x 2 Kb (1 - Kb) / Kg,
 *   b = 0.299 x 2 (1 - Kr) - 0.587 x 2 Kr (1 - Kr) / Kg
 * (BT.709: a = 0.10158, b = 0.19608; BT.601: both 0, by this header's
 * definition), so these frames cost the forward row kernel a read of the
 * half-resolution chroma plane next to the luma plane (1.5 samples per pixel
 * instead of 1).  The I and Q rows of RGBToYIQ sum to 0, so (I, Q) stays a
 * 2 x 2 matrix of (cb, cr) (mm_ycbcr_matrix); neutral chroma still gives
 * exactly zero I and Q and luma = y.
 * Out of scope: PQ / HLG transfer curves (the samples are taken as they are,
 * like every other format's), constant-luminance BT.2020, 4:4:4 and planar or
 * P210 4:2:2 (packed 4:2:2: MM_YUY2 / MM_UYVY and, 10-bit, MM_Y210 below),
 * chroma siting other than the shared 2 x 2 sample, odd sizes. */
#define MM_MATRIX_BT709   32   /* Kr 0.2126, Kb 0.0722 */
#define MM_MATRIX_BT2020  64   /* Kr 0.2627, Kb 0.0593, non-constant luminance */

/* Grayscale camera frames (backward-compatible addition to ABI 10: a caller
 * detects it by mm_frame_bytes(W, H, MM_Y8, &n) == MM_OK).  One plane, one
 * sample per pixel, as a machine-vision camera (GenICam Mono8 / Mono10 /
 * Mono12 / Mono16), a thermal imager or a grayscale decoder stores it, tightly
 * packed: H rows of W bytes (MM_Y8, W H bytes in all) or of W little-endian
 * 16-bit words with the code in the LOW bits (MM_Y10 / MM_Y12 / MM_Y16, 2 W H
 * bytes: ffmpeg's gray10le / gray12le / gray16le); frame k of a stream at
 * k * mm_frame_bytes.  With max = 255, 1023, 4095 or 65535:
 *   in:  the frame IS the RGBA32F frame R = G = B = v = sample / max, alpha 1.
 *        v is NOT clamped: a Y10 / Y12 word above max gives v > 1, which
 *        passes until the reference's saturate, like an HDR value.
 *        RGBToYIQ's luma row sums to 1 and its I and Q rows to 0, so the luma
 *        of the pixel is the sample and (I, Q) is zero;
 *   out: of the reference's saturated RGB, Yl = 0.299 R + 0.587 G + 0.114 B,
 *        code = floor(Yl max + 0.5) clamped to 0..max (for the kernels: the
 *        code of the saturated magnified luma, since R = G = B); the bits of
 *        a Y10 / Y12 output word above the code are zero.
 * The first frame after mm_create / mm_reset and apply_magnification = 0 pass
 * the W x H samples through bitwise, stray high bits of Y10 / Y12 words
 * included; padding stays untouched.  There is no chroma subsampling, so odd W
 * and H are supported, in every mode (pyramid, standard, steerable), and so
 * are show_magnitude / show_phase, split screen included: the views are
 * R-channel pictures and the output code is the view's R value, encoded as
 * above.  A matrix bit on these codes is MM_ERR_INVALID (there is no matrix);
 * in_layout->format == out_layout->format holds as everywhere.
 * Surfaces: the unit u is 1 for MM_Y8 and 2 for the word formats;
 * chroma_offset = chroma_pitch = 0 (else MM_ERR_INVALID); device frame
 * pointers, pitch and frame stride are multiples of u; the extent and 4 GiB
 * rules are unchanged.  The fused kernels' wide stores (four bytes as a dword,
 * four words as 8 bytes) run where every output row of the call is 4-byte
 * aligned; any other layout takes the unfused pair, same results.
 * The operator changes luma only, so this is the cheapest path of the
 * library: the forward kernel reads the plane as it reads a 4:2:0 frame's
 * luma plane, the compose stage reads nothing from the input at all, and 1 or
 * 2 bytes per pixel travel each way.
 * Out of scope: packed Mono10p / Mono12p; MSB-aligned words (a P016-style mono
 * plane); limited-range mono; Bayer mosaics; the ring entry points
 * (include/mm_ring.h), which stay RGBA8 / RGBA32F as for NV12; the Unity shim. */
#define MM_Y8   8    /* 1 B/px, full range: v = byte / 255                          */
#define MM_Y10  9    /* 2 B/px, little-endian word, code in the LOW 10 bits: v = word / 1023 */
#define MM_Y12  10   /* ... low 12 bits: v = word / 4095                            */
#define MM_Y16  11   /* ... v = word / 65535                                        */

/* Packed 4:2:2 capture frames (backward-compatible addition to ABI 10: a
 * caller detects it by mm_frame_bytes(W, H, MM_YUY2, &n) == MM_OK).  8-bit
 * Y'CbCr 4:2:2 as a live source hands it out: UVC webcams and most USB capture
 * devices deliver YUY2 (V4L2 YUYV, ffmpeg yuyv422), SDI / HDMI capture cards
 * and QuickTime 2vuy deliver UYVY (V4L2 UYVY, ffmpeg uyvy422).  One plane,
 * tightly packed: H rows of W / 2 four-byte macropixels, bytes Y0 Cb Y1 Cr
 * (MM_YUY2) or Cb Y0 Cr Y1 (MM_UYVY), 2 W bytes per row and 2 W H per frame;
 * frame k of a stream at k * mm_frame_bytes.  W and H even (else
 * MM_ERR_UNSUPPORTED from mm_frame_bytes, mm_surface_* and every frame entry
 * point; 4:2:2 itself would allow odd H, which is left out);
 * show_magnitude / show_phase are refused with MM_ERR_UNSUPPORTED, as for NV12.
 * MM_MATRIX_BT709 / MM_MATRIX_BT2020 may be OR-ed on exactly as on the 4:2:0
 * codes: the valid formats are 24..27 (BT.601), 56..59 and 88..91; codes
 * 28..31 stay unknown (the 10-bit form lives at 22 / 23: MM_Y210 below).
 * The codes and ranges are NV12's, the matrices the matrix bits', and a chroma
 * sample is shared by its 1 x 2 pixels.  The frame IS the RGBA32F frame of
 * this decode and the result the reference's result on it:
 *   in:  y = (Y - 16) / 219, cb = (Cb - 128) / 224, cr = (Cr - 128) / 224
 *        (_FULL: Y / 255, (C - 128) / 255); R, G, B by the format's decode:
 *        BT.601 with the six-digit coefficients of the NV12 section, a matrix
 *        bit with the (Kr, Kb) form of the matrix section; alpha 1, NOT
 *        clamped;
 *   out: of the saturated RGB, Y', Cb', Cr' by the format's weights; luma code
 *        per pixel, chroma code 128 + scale x the mean of the macropixel's two
 *        pixels' C'; codes floor(v + 0.5) clamped to 0..255.
 * The first frame after mm_create / mm_reset and apply_magnification = 0 pass
 * all 2 W H bytes through bitwise.  mm_ycbcr_matrix accepts these codes (the
 * values of the 4:2:0 code of the same matrix); mm_nv12_chroma_matrix is
 * unchanged.  For BT.601 frames the forward row kernel uses the luma bytes
 * alone (every second byte; the chroma byte loaded beside each is dropped);
 * matrixed frames cost it one dword per pixel and source row, which holds Y,
 * Cb and Cr.  2 bytes per pixel travel each way and the
 * host converts nothing; against NV12 the vertical chroma resolution is kept.
 * Surfaces: the unit u is 4, one macropixel; chroma_offset = chroma_pitch = 0
 * (else MM_ERR_INVALID); pitch >= 2 W; device frame pointers, pitch and frame
 * stride are multiples of 4, so a region of interest starts on an even column;
 * the extent and 4 GiB rules are unchanged.  Every row of every legal layout
 * is dword aligned, so the fused kernels run under their geometry conditions
 * alone.
 * Out of scope: P210 (10-bit packed 4:2:2 is MM_Y210 and MM_V210 below); planar 4:2:2 and 4:4:4 on the
 * device; odd H; the debug views; chroma siting other than the shared 1 x 2
 * sample; PQ / HLG; the ring entry points (include/mm_ring.h); the Unity shim;
 * a host 4:2:2 to RGBA conversion. */
#define MM_YUY2      24   /* 8-bit packed 4:2:2, bytes Y0 Cb Y1 Cr, BT.601 limited range */
#define MM_YUY2_FULL 25   /* the same, full range */
#define MM_UYVY      26   /* bytes Cb Y0 Cr Y1, BT.601 limited range */
#define MM_UYVY_FULL 27   /* the same, full range */

/* 10-bit packed 4:2:2 frames (backward-compatible addition to ABI 10: a caller
 * detects it by mm_frame_bytes(W, H, MM_Y210, &n) == MM_OK).  The frame of the
 * sources where bit depth matters most: SDI / HDMI capture SDKs offer it beside
 * v210, HEVC 4:2:2 10-bit, ProRes and DNxHR decodes produce it; DirectX / Media
 * Foundation, VA-API and ffmpeg (y210le) call it Y210: the YUY2 macropixel in
 * 16-bit words, the code in the high bits exactly as P010 stores its samples.
 * One plane, tightly packed: H rows of W / 2 eight-byte macropixels, four
 * little-endian 16-bit words Y0 Cb Y1 Cr, 4 W bytes per row and 4 W H per
 * frame (1920 x 1080: 8,294,400 bytes, pitch 7,680); frame k of a stream at
 * k * mm_frame_bytes.  As in P010 the word is read as 16-bit fixed point,
 * v = word / 64 in 10-bit code units: Y210 content has the low 6 bits zero, a
 * Y216 surface is accepted as it is and its low bits are honoured.  W and H
 * even (else MM_ERR_UNSUPPORTED from mm_frame_bytes, mm_surface_* and every
 * frame entry point); show_magnitude / show_phase are refused with
 * MM_ERR_UNSUPPORTED.  MM_MATRIX_BT709 / MM_MATRIX_BT2020 may be OR-ed on: the
 * valid formats are 22, 23 (BT.601), 54, 55 and 86, 87; both bits together or
 * any other stray bit give MM_ERR_INVALID before anything is queued.  Codes
 * 20 and 21 stay unknown.
 * The ranges are P010's, the matrices the matrix bits', and a chroma sample is
 * shared by its 1 x 2 pixels.  The frame IS the RGBA32F frame of this decode
 * and the result the reference's result on it:
 *   in:  y = (v - 64) / 876, cb = (v - 512) / 896, cr = (v - 512) / 896
 *        (_FULL: v / 1023, (v - 512) / 1023); R, G, B by the format's decode:
 *        BT.601 with the six-digit coefficients of the NV12 section, a matrix
 *        bit with the (Kr, Kb) form of the matrix section; alpha 1, NOT
 *        clamped;
 *   out: of the saturated RGB, Y', Cb', Cr' by the format's weights; luma code
 *        per pixel, chroma code 512 + scale x the mean of the macropixel's two
 *        pixels' C'; codes floor(v + 0.5) clamped to 0..1023, stored as
 *        code << 6: the low 6 bits of every output word are zero.
 * The first frame after mm_create / mm_reset and apply_magnification = 0 pass
 * all 4 W H bytes through bitwise, low bits included.  mm_ycbcr_matrix accepts
 * these codes (the values of the 4:2:0 code of the same matrix).  For BT.601
 * frames the forward row kernel uses the luma words alone (the chroma word
 * loaded beside each is dropped) and the state is bitwise that of a P010 frame
 * with the same luma words; matrixed frames cost it one 8-byte macropixel per
 * pixel and source row.  4 bytes per pixel travel each way and the host
 * converts nothing; against P010 the vertical chroma resolution is kept,
 * against MM_YUY2 the two bits that phase_scale would amplify as noise.
 * in_layout->format == out_layout->format, as everywhere.
 * Surfaces: the unit u is 8, one macropixel; chroma_offset = chroma_pitch = 0
 * (else MM_ERR_INVALID); pitch >= 4 W; device frame pointers, pitch and frame
 * stride are multiples of 8, so a region of interest starts on an even column;
 * the extent and 4 GiB rules are unchanged.  mm_surface_aligned(1920, 1080,
 * MM_Y210, 256, 16) has pitch 7,680 and frame_stride 8,355,840; with
 * pitch_align 1024 the pitch is 8,192.  The fused kernels' 16-byte quads (two
 * macropixels) are 16-byte aligned where base, pitch and stride are, and
 * multi-dword accesses at 8-byte-aligned addresses in any other legal layout:
 * the fused kernels run under their geometry conditions alone.
 * (v210, three 10-bit samples per 32-bit word, is MM_V210 below.)
 * Out of scope: v216 / a UYVY
 * word order (codes 28..31 stay unknown); P210 and planar 4:2:2; Y410 / 4:4:4;
 * low-bit-aligned words; odd H; the debug views; chroma siting other than the
 * shared 1 x 2 sample; PQ / HLG; the ring entry points (include/mm_ring.h);
 * the Unity shim; a host 4:2:2 to RGBA conversion. */
#define MM_Y210      22   /* 10-bit packed 4:2:2, words Y0 Cb Y1 Cr, BT.601 limited range */
#define MM_Y210_FULL 23   /* the same, full range */

/* Packed RGB frames (a backward-compatible addition to ABI 10: a caller
 * detects it by mm_frame_bytes(W, H, MM_RGB24, &n) == MM_OK).  What Python and
 * desktop imaging hand out: cv2.VideoCapture / cv2.imread (in B, G, R order),
 * PIL, imageio, torchvision, ffmpeg's rgb24 / bgr24, binary PPM: [H, W, 3]
 * bytes.  One plane, tightly packed: H rows of W three-byte pixels, bytes
 * R G B (MM_RGB24) or B G R (MM_BGR24 = MM_RGB24 | MM_ORDER_BGR), 3 W bytes per
 * row and 3 W H per frame (1920 x 1080: 6,220,800 bytes, pitch 5,760); frame k
 * of a stream at k * mm_frame_bytes.  There is no alpha byte and no
 * subsampling: every size the RGBA formats take, odd W and H included, every
 * mode (pyramid, standard, steerable) and the debug views.
 * The frame IS the RGBA32F frame R, G, B = byte / 255, alpha 1, equivalently
 * the MM_RGBA8 frame with the same colour bytes and alpha 255, and the result
 * the reference's result on it:
 *   in:  v = byte / 255 per channel, as MM_RGBA8;
 *   out: round(saturate(v) * 255) per channel, MM_RGBA8's rule, three bytes.
 * Two identities hold bitwise, in every mode, view, call form and layout:
 *   1. the output bytes are the MM_RGBA8 path's R, G, B bytes on that frame,
 *      and the temporal state (mm_get_state / mm_compute_state) is bitwise
 *      that MM_RGBA8 frame's (the operator gives alpha weight 0 everywhere);
 *   2. MM_BGR24 on the byte-swapped frame gives the byte-swapped output of
 *      MM_RGB24, and the same state.
 * A debug view's output is the MM_RGBA8 view's R, G, B bytes (R the view's
 * value, G = B = 0, in the frame's byte order).  The first frame after
 * mm_create / mm_reset and apply_magnification = 0 pass all 3 W H bytes through
 * bitwise.  in_layout->format == out_layout->format, as everywhere: MM_RGB24
 * in with MM_BGR24 out is MM_ERR_INVALID.
 * The byte-order bit is valid on MM_RGB24 alone: MM_RGBA8 | 128,
 * MM_RGBA8_SRGB | 128, the bit on any Y'CbCr or single-plane code, code 14, a
 * matrix bit on 13 or 141 (45, 77, 173), any other stray bit (13 | 256) and
 * negative codes are MM_ERR_INVALID from mm_frame_bytes, mm_surface_* and every
 * frame entry point, before anything is queued.
 * Surfaces: the unit u is 1: a real [H, W, 3] array and any region of interest
 * of one start at any byte; chroma_offset = chroma_pitch = 0 (else
 * MM_ERR_INVALID); pitch >= 3 W, any value; device frame pointers and
 * frame_stride need no alignment (frame_stride >= extent when count > 1); the
 * extent and 4 GiB rules are unchanged.  mm_surface_aligned(1920, 1080,
 * MM_RGB24, 256, 16) has pitch 5,888 and frame_stride 6,406,144;
 * mm_surface_aligned(97, 63, MM_RGB24, 256, 16) has pitch 512, frame_stride
 * 32,768 and extent 32,035.  Padding is never read and never written, the byte
 * after a row's last pixel included.  The fused kernels' quads (four pixels,
 * 12 bytes, one 12-byte load and one 12-byte store at a 4-byte-aligned
 * address) run where base, pitch and, past one frame, frame_stride are
 * multiples of 4 on both sides (every tight frame with W % 8 == 0); any other
 * legal layout takes the unfused kernels: the same bytes.  3 bytes per pixel
 * travel each way and nobody widens a frame to RGBA8 or strips an alpha.
 * Out of scope here: BGRA8 / BGRA8 sRGB, which are formats of their own
 * (MM_ORDER_BGRA, "BGRA frames" below: MM_ORDER_BGR on MM_RGBA8 / MM_RGBA8_SRGB
 * stays MM_ERR_INVALID, because every code below 4096 that was no format stays
 * none); RGB48; planar RGB; an
 * sRGB-decoded RGB24; MM_RGB24 in with MM_BGR24 out; the LDS-DMA staging of the
 * fused kernels' source rows (MM_RGBA8's alone: 4-byte pixels); the ring
 * entry points (include/mm_ring.h); the Unity shim; mm_extmem_check. */
#define MM_RGB24     13    /* 3 B/px, bytes R G B, UNORM as MM_RGBA8, no alpha */
#define MM_ORDER_BGR 128   /* byte-order bit: B G R */
#define MM_BGR24     (MM_RGB24 | MM_ORDER_BGR)   /* 141 */

/* Three-plane 4:2:0 frames (backward-compatible addition to ABI 10: a caller
 * detects it by mm_frame_bytes(W, H, MM_I420, &n) == MM_OK).  What every
 * software decoder (libavcodec, libvpx, dav1d), WebRTC's frame buffers, the
 * x264 / x265 / SVT encoder inputs and every C420 .y4m file hold: I420, ffmpeg's
 * yuv420p.  Tightly packed: H rows of W luma bytes, then H/2 rows of W/2 Cb
 * bytes, then H/2 rows of W/2 Cr bytes, W H 3/2 bytes in all (the frame payload
 * of a C420 .y4m as it lies in the file); frame k of a stream at
 * k * mm_frame_bytes.  MM_PLANAR is a plane-layout bit beside the matrix and
 * order bits: MM_I420 = MM_NV12 | MM_PLANAR, and a matrix bit may be OR-ed on
 * as on NV12.  The valid codes are 528, 529, 560, 561, 592 and 593.
 * The bit is valid on the two NV12 codes alone (and, together with
 * MM_LOW_BITS, on the two P010 codes: MM_I010 below): MM_PLANAR by itself, the
 * bit on an RGBA, single-plane, P010, packed 4:2:2, MM_Y210 or packed RGB code,
 * the bit together with MM_ORDER_BGR, both matrix bits together and any other
 * stray bit (528 | 256, 528 | 1024) are MM_ERR_INVALID from mm_frame_bytes,
 * mm_surface_* and every frame entry point, before anything is queued.
 * Restrictions, all NV12's: W and H even (else MM_ERR_UNSUPPORTED);
 * show_magnitude / show_phase are refused with MM_ERR_UNSUPPORTED;
 * in_layout->format == out_layout->format.
 * The semantics are NV12's word for word (ranges, matrices, the chroma sample
 * shared by its 2 x 2 pixels, the out rule, rounding and clamps): an I420 frame
 * IS the NV12 frame with the same samples, and where a pixel's two chroma
 * samples lie is a matter of loads and stores.  Two identities hold bitwise, in
 * every mode (pyramid, standard, steerable), call form (single, stream,
 * host-memory frames), batch size, edge mode and layout:
 *   1. the output is the NV12 path's output on the interleaved frame,
 *      de-interleaved;
 *   2. the temporal state (mm_get_state / mm_compute_state) is bitwise that
 *      NV12 frame's.
 * The first frame after mm_create / mm_reset and apply_magnification = 0 pass
 * all W H 3/2 bytes through bitwise.
 * Surfaces: mm_surface has one chroma offset, so the third plane's place is
 * derived.  pitch is the luma pitch, chroma_offset the Cb plane's offset,
 * chroma_pitch the pitch of a Cb row and of a Cr row alike, and THE Cr PLANE
 * STARTS chroma_pitch x H/2 BYTES AFTER THE Cb PLANE.  The unit u is 1: frame
 * pointers, pitches and strides need no alignment (W = 98 has chroma rows of 49
 * bytes).  pitch >= W; chroma_pitch >= W/2; chroma_offset at or past the end of
 * the last luma row's samples; the extent is the byte after the last Cr sample,
 * at most 2^32; frame_stride >= extent when count > 1; size_t overflows are
 * MM_ERR_INVALID; padding is never read and never written.
 * mm_surface_tight(1920, 1080, MM_I420): pitch 1,920, chroma_offset 2,073,600,
 * chroma_pitch 960, frame_stride 3,110,400.  mm_surface_tight(98, 62, MM_I420):
 * pitch 98, chroma_offset 6,076, chroma_pitch 49 (the Cr plane at 7,595),
 * frame_stride 9,114.  mm_surface_aligned: the luma pitch is W rounded up to
 * pitch_align, chroma_pitch = pitch / 2 (MM_ERR_INVALID where that pitch is
 * odd), rows_align even, chroma_offset = pitch x padded rows, frame_stride =
 * pitch x padded rows x 3/2: mm_surface_aligned(1920, 1080, MM_I420, 256, 16)
 * has pitch 2,048, chroma_offset 2,228,224, chroma_pitch 1,024 (the Cr plane at
 * 2,781,184), frame_stride 3,342,336 and extent 3,334,080.
 * The fused kernels move a quad's two Cb and two Cr samples as one 2-byte
 * access per plane and its four luma codes as one dword: they run where the
 * output's luma rows lie on multiples of 4 and every Cb and Cr row of every
 * frame of the launch on a multiple of 2, on both sides (every tight frame
 * with W % 8 == 0); any other legal layout takes the unfused kernels, whose
 * chroma accesses are single bytes: the same bytes.
 * mm_ycbcr_matrix takes the six codes and returns the NV12 code's values;
 * mm_convert_supported(x, x) is MM_OK for them and any mixed pair with a planar
 * code MM_ERR_UNSUPPORTED; mm_compute_state* takes them.
 * Out of scope: YV12 (the Cr plane first); planes at independent addresses or
 * with padded chroma rows between them (a region of interest narrower in
 * height than its parent needs that); planar 4:2:2 / 4:4:4 (10-bit three-plane
 * 4:2:0, yuv420p10le, is MM_I010 below); any mixed convert pair; the ring
 * entry points (include/mm_ring.h), the Unity shim and mm_extmem_check; odd
 * sizes and the debug views. */
#define MM_PLANAR    512                          /* plane-layout bit: Cb and Cr in planes of their own */
#define MM_I420      (MM_NV12 | MM_PLANAR)        /* 528 */
#define MM_I420_FULL (MM_NV12_FULL | MM_PLANAR)   /* 529 */

/* 10-bit three-plane 4:2:0 frames (backward-compatible addition to ABI 10: a
 * caller detects it by mm_frame_bytes(W, H, MM_I010, &n) == MM_OK).  What a
 * software decoder produces for 10-bit content (libavcodec, dav1d, libvpx on
 * HEVC Main10, AV1 10-bit, VP9 profile 2), what the x265 and SVT 10-bit inputs
 * take and what every C420p10 .y4m file holds: ffmpeg's yuv420p10le, I010 in
 * libyuv and VLC.  Three planes of little-endian 16-bit words with the code in
 * the word's LOW 10 bits, tightly packed: H rows of W luma words, then H/2 rows
 * of W/2 Cb words, then H/2 rows of W/2 Cr words, 3 W H bytes in all (6,220,800
 * at 1920 x 1080, 18,228 at 98 x 62: the frame payload of a C420p10 .y4m as it
 * lies in the file); frame k of a stream at k * mm_frame_bytes.
 * MM_LOW_BITS is one more bit beside the matrix, order and plane bits: the code
 * sits in the word's low bits.  MM_I010 = MM_P010 | MM_PLANAR | MM_LOW_BITS, and
 * a matrix bit may be OR-ed on as on P010.  The valid codes are 1554, 1555,
 * 1586, 1587, 1618 and 1619.  The bit is valid only together with MM_PLANAR on
 * the two P010 codes: MM_LOW_BITS by itself, 18 | 512 and 19 | 512 without it
 * (high-bit words in three planes: a layout nobody produces), 528 | 1024,
 * 18 | 1024, the bit on any other family, the bit with MM_ORDER_BGR, both matrix
 * bits and any other stray bit (1554 | 256, 1554 | 2048) are MM_ERR_INVALID from
 * mm_frame_bytes, mm_surface_* and every frame entry point, before anything is
 * queued.
 * Restrictions, P010's and I420's: W and H even (else MM_ERR_UNSUPPORTED);
 * show_magnitude / show_phase are refused with MM_ERR_UNSUPPORTED;
 * in_layout->format == out_layout->format.
 * The semantics are P010's word for word with v = word in 10-bit code units
 * instead of word / 64 (ranges, matrices, the chroma sample shared by its 2 x 2
 * pixels, the out rule, rounding and clamps).  Output words hold the code in
 * the low 10 bits and their high 6 bits are zero.  The word is neither masked
 * nor clamped on input: a word above 1023 gives v > 1023 and passes until the
 * reference's saturate, as MM_Y10 treats its words.  The first frame after
 * mm_create / mm_reset and apply_magnification = 0 pass all 3 W H bytes through
 * bitwise, stray high bits included.
 * Three identities hold bitwise:
 *   1. for frames whose words are all <= 1023, the output is the MM_P010
 *      path's output on the frame word << 6 with Cb and Cr interleaved, shifted
 *      right by 6 and de-interleaved, in every mode (pyramid, standard,
 *      steerable), call form, batch size, edge mode and layout;
 *   2. the temporal state (mm_get_state / mm_compute_state*) is bitwise that
 *      P010 frame's (the word unit is a power of two, so every input-side
 *      uniform scales exactly);
 *   3. the state of an MM_I010_FULL frame is bitwise the state of the MM_Y10
 *      frame that is its luma plane (a surface of the same buffer), with luma
 *      words above 1023 too.
 * Surfaces: as MM_I420 in words.  pitch is the luma pitch, chroma_offset the Cb
 * plane's offset, chroma_pitch the pitch of a Cb row and of a Cr row alike, and
 * the Cr plane starts chroma_pitch x H/2 bytes after the Cb plane.  The unit u
 * is 2: device frame pointers, pitch, chroma_offset, chroma_pitch and
 * frame_stride are multiples of 2.  pitch >= 2 W; chroma_pitch >= W (the bytes
 * of W/2 words); chroma_offset at or past the end of the last luma row's
 * samples; the extent is the byte after the last Cr sample, at most 2^32;
 * frame_stride >= extent when count > 1; size_t overflows are MM_ERR_INVALID;
 * padding is never read and never written.
 * mm_surface_tight(1920, 1080, MM_I010): pitch 3,840, chroma_offset 4,147,200,
 * chroma_pitch 1,920 (the Cr plane at 5,184,000), frame_stride 6,220,800.
 * mm_surface_tight(98, 62, MM_I010): pitch 196, chroma_offset 12,152,
 * chroma_pitch 98 (the Cr plane at 15,190), frame_stride 18,228.
 * mm_surface_aligned: the luma pitch is 2 W rounded up to pitch_align,
 * chroma_pitch = pitch / 2 (MM_ERR_INVALID where that is odd), rows_align even:
 * mm_surface_aligned(1920, 1080, MM_I010, 256, 16) has pitch 3,840,
 * chroma_offset 4,177,920, chroma_pitch 1,920 (the Cr plane at 5,214,720),
 * frame_stride 6,266,880 and extent 6,251,520.
 * The fused kernels move a quad's two Cb words and its two Cr words as one
 * dword per plane and its four luma codes as one 8-byte store at a
 * dword-aligned address: they run where the output's luma rows and every Cb and
 * Cr row of every frame of the launch lie on multiples of 4, on both sides
 * (every tight frame with W % 8 == 0, the decoder layout); any other legal
 * layout takes the unfused kernels, whose accesses are single words: the same
 * bytes.
 * mm_ycbcr_matrix takes the six codes and returns the P010 code's values;
 * mm_convert_supported(x, x) is MM_OK for them and any mixed pair with one of
 * them MM_ERR_UNSUPPORTED; mm_compute_state* takes them.
 * Out of scope: 12-bit planar (yuv420p12le), yuv422p10le and yuv444p10le; the
 * Cr plane first; planes at independent addresses; any mixed convert pair; the
 * ring entry points (include/mm_ring.h), the Unity shim and mm_extmem_check;
 * odd sizes and the debug views; PQ / HLG. */
#define MM_LOW_BITS  1024                                        /* word-alignment bit: the code in the word's low bits */
#define MM_I010      (MM_P010 | MM_PLANAR | MM_LOW_BITS)         /* 1554 */
#define MM_I010_FULL (MM_P010_FULL | MM_PLANAR | MM_LOW_BITS)    /* 1555 */

/* v210 capture frames (backward-compatible addition to ABI 10: a caller detects
 * it by mm_frame_bytes(W, H, MM_V210, &n) == MM_OK).  The 10-bit frame SDI and
 * HDMI capture cards deliver by default: every DeckLink, AJA and Bluefish SDK
 * offers it as the 10-bit mode, QuickTime, AVI and MXF "uncompressed 10-bit"
 * files hold it, ffmpeg's v210 codec reads and writes it.  MM_Y210's samples at
 * 2.67 instead of 4 bytes per pixel: each little-endian dword holds three
 * 10-bit codes in bits 0-9, 10-19 and 20-29 (bits 30-31 unused), and six
 * pixels make a group of four dwords:
 *     dword 0:  Cb(0,1)  Y0       Cr(0,1)        (low, middle, high field)
 *     dword 1:  Y1       Cb(2,3)  Y2
 *     dword 2:  Cr(2,3)  Y3       Cb(4,5)
 *     dword 3:  Y4       Cr(4,5)  Y5
 * (Cb, Y, Cr, Y, ... = 1 .. 12 in this order: 0x00300801, 0x00601404,
 * 0x00902007, 0x00C02C0A.)  The format is the pack bit MM_PACK_V210 on a Y210
 * code: MM_V210 = MM_Y210 | 4096 (4118), MM_V210_FULL (4119), with one matrix
 * bit 4150, 4151, 4182, 4183 (4096: every code below it that is no format
 * stays MM_ERR_INVALID).  The bit alone, on any other family, with
 * MM_ORDER_BGR, MM_PLANAR, MM_LOW_BITS, both matrix bits or 256 is
 * MM_ERR_INVALID from mm_frame_bytes, mm_surface_* and every frame entry point,
 * before anything is queued.
 * Semantics are MM_Y210's word for word with v = the 10-bit code: a V210 frame
 * IS the MM_Y210 frame whose words are code << 6 (P010's ranges, the matrix
 * bits' matrices, the shared 1 x 2 chroma sample, the out rule, rounding and
 * clamps), so the output is bitwise the Y210 path's on the unpacked frame,
 * packed again, and the temporal state (mm_get_state / mm_compute_state*)
 * bitwise that frame's.  On input bits 30-31 and the unused fields of a partial
 * last group are ignored; output dwords have bits 30-31 zero and the unused
 * fields of a written dword zero.  The first frame and apply_magnification = 0
 * pass every used dword through bitwise, stray bits included.  W and H even
 * (else MM_ERR_UNSUPPORTED); no debug views; in_layout->format ==
 * out_layout->format; mm_convert_supported(x, x) is MM_OK and any mixed pair
 * MM_ERR_UNSUPPORTED; mm_ycbcr_matrix takes the six codes and returns the Y210
 * code's values.
 * Rows: the used dwords of a row are D(W) = 4 (W / 6) + {0, 2, 3}[(W % 6) / 2],
 * so a row is 4 D(W) bytes (1920: 5,120; 1280: 3,416; 98: 264; 64: 172).
 * mm_surface_tight / mm_frame_bytes use the pitch every SDK and ffmpeg use,
 * 128 ceil(W / 48): 1920 x 1080 has pitch 5,120 and 5,529,600 bytes, 1280 x 720
 * pitch 3,456 and 2,488,320 bytes, 98 x 62 pitch 384 and 23,808 bytes; frame k
 * of a stream at k * mm_frame_bytes.  Everything past a row's 4 D(W) bytes is
 * padding, never read and never written, in the tight frame too.
 * Surfaces: the unit u is 16, one group; device frame pointers, pitch and frame
 * stride are multiples of 16; pitch >= 4 D(W); chroma_offset = chroma_pitch = 0;
 * the extent is pitch (H - 1) + 4 D(W); the 4 GiB and overflow rules are
 * unchanged; a region of interest starts on a column that is a multiple of 6.
 * mm_surface_aligned(1920, 1080, MM_V210, 256, 16): pitch 5,120, frame_stride
 * 5,570,560; mm_surface_aligned(1280, 720, MM_V210, 128, 1): pitch 3,456.
 * The forward row kernel loads one dword per tap (BT.601) or the pixel pair's
 * two dwords (a matrix bit); the compose is always the unfused pair, its
 * groups stored whole (16 bytes, or a partial last group's 8 or 12).
 * Out of scope: a fused compose; convert pairs; v216 and a UYVY word order;
 * P210 and planar 4:2:2; odd sizes and the debug views; regions of interest not
 * on a multiple of 6 columns; other chroma sitings; PQ / HLG; the ring entry
 * points (include/mm_ring.h), the Unity shim and mm_extmem_check. */
#define MM_PACK_V210 4096                                        /* packing bit: three 10-bit codes per dword */
#define MM_V210      (MM_Y210 | MM_PACK_V210)                    /* 4118 */
#define MM_V210_FULL (MM_Y210_FULL | MM_PACK_V210)               /* 4119 */

/* BGRA frames (a backward-compatible addition to ABI 10: a caller detects it by
 * mm_frame_bytes(W, H, MM_BGRA8, &n) == MM_OK).  The four-byte pixel B G R A
 * that desktop, capture and display paths hand out: D3D and Vulkan swap chains
 * and DXGI desktop duplication (B8G8R8A8_UNORM / _SRGB), CoreVideo's 32BGRA,
 * NDI's BGRA / BGRX, DeckLink's 8-bit BGRA mode, GDI, Qt's Format_ARGB32, Cairo,
 * libyuv's and WebRTC's "ARGB", OpenCV's four-channel mats.  The format is the
 * byte-order bit MM_ORDER_BGRA on a 4-byte UNORM code: MM_BGRA8 = MM_RGBA8 |
 * 8192 (8192), MM_BGRA8_SRGB = MM_RGBA8_SRGB | 8192 (8195).  Sizes, modes,
 * views and call forms are MM_RGBA8's: 4 W bytes per row and 4 W H per frame,
 * odd W and H, pyramid, standard and steerable mode, the debug views.
 * A BGRA frame IS the MM_RGBA8 (MM_RGBA8_SRGB) frame with bytes 0 and 2 of every
 * pixel exchanged; byte 3 is alpha.  BGRX is the same format: the operator gives
 * alpha weight 0, and the output alpha after the first frame is 255.  With
 * swap() for that exchange, three identities hold bitwise, in every mode, view
 * (the split screen included), call form (single, stream, host-memory, lanes),
 * edge mode, batch size, size and layout:
 *   1. out_BGRA8(x) == swap(out_RGBA8(swap(x))), alpha byte included, and the
 *      same for the sRGB pair (a debug view's value lies in byte 2);
 *   2. the temporal state (mm_get_state, mm_compute_state*, a lane's state) is
 *      bitwise that RGBA8 frame's;
 *   3. the first frame after mm_create / mm_reset and apply_magnification = 0
 *      pass all 4 W H bytes through bitwise.  Padding is never read or written.
 * The bit is valid on codes 0 and 3 alone: 8193 and 8194 (float BGRA: nobody
 * produces it), the bit on any Y'CbCr, single-plane, packed RGB, planar or v210
 * code, the bit together with MM_ORDER_BGR, a matrix bit, MM_PLANAR,
 * MM_LOW_BITS, MM_PACK_V210 or 256, 16384 and every higher stray bit, and
 * negative codes are MM_ERR_INVALID from mm_frame_bytes, mm_surface_* and every
 * frame entry point, before anything is queued.  (MM_RGBA8 | 128 stays
 * MM_ERR_INVALID too: see "Packed RGB frames".)  mm_ycbcr_matrix refuses both
 * codes, as it does MM_RGBA8.
 * Surfaces: the unit u is 4 and every rule is MM_RGBA8's: chroma_offset =
 * chroma_pitch = 0 (else MM_ERR_INVALID), pitch >= 4 W, device frame pointers,
 * pitch and frame_stride multiples of 4.  mm_surface_tight and
 * mm_surface_aligned return MM_RGBA8's numbers with the BGRA code:
 * mm_surface_aligned(1920, 1080, MM_BGRA8, 256, 16) has pitch 7,680 and
 * frame_stride 8,355,840, mm_surface_aligned(97, 63, MM_BGRA8, 256, 16) pitch
 * 512 and frame_stride 32,768.  The fused kernels and the LDS-DMA staging of
 * their source rows run under exactly MM_RGBA8's conditions.
 * in_layout->format == out_layout->format, as everywhere: MM_RGBA8 in with
 * MM_BGRA8 out is MM_ERR_INVALID from the same-format entry points and
 * MM_ERR_UNSUPPORTED from mm_convert_supported.
 * Convert pairs (see "Different formats in and out"), what a display path and a
 * screen-capture encoder need: any MM_NV12 or MM_P010 code in with MM_BGRA8
 * out, and MM_BGRA8 in with any MM_NV12 code out.  Bitwise,
 * X -> BGRA8 == swap(X -> RGBA8) and BGRA8 -> NV12 (x) == RGBA8 -> NV12
 * (swap(x)); the state is the in format's; passthrough frames are the plain
 * conversion.  MM_BGRA8_SRGB has no mixed pair, as MM_RGBA8_SRGB has none.
 * The exchange is made where the kernels are compiled (instances of their own,
 * which name other bytes and constants in the same instructions), so a BGRA
 * frame costs what its RGBA8 twin costs and nobody swizzles a frame.
 * Out of scope: float BGRA; ARGB / ABGR byte orders; BGR-ordered 10-bit
 * (A2R10G10B10); RGBA8 <-> BGRA8 and RGB24 <-> BGRA8 transcodes; MM_BGRA8_SRGB
 * in a mixed pair; P010 out; mm_synth_frames (it stays MM_RGBA8); the ring entry
 * points (include/mm_ring.h), the Unity shim and mm_extmem_check. */
#define MM_ORDER_BGRA 8192                             /* byte-order bit of the 4-byte UNORM formats: B G R A */
#define MM_BGRA8      (MM_RGBA8 | MM_ORDER_BGRA)       /* 8192 */
#define MM_BGRA8_SRGB (MM_RGBA8_SRGB | MM_ORDER_BGRA)  /* 8195 */

/* mm_params.mode */
#define MM_MODE_PYRAMID   0  /* usePyramidDecomposition = true (.cs:18, :128-131) */
#define MM_MODE_STANDARD  1   /* usePyramidDecomposition = false (.cs:132-135, :208-232) */
#define MM_MODE_STEERABLE 2  /* extension f2: oriented local-phase subbands + temporal filter */
#define MM_FILTER_DIFF 0      /* steerable: the reference's 2-tap phase difference per coefficient */
#define MM_FILTER_IIR  1      /* steerable: band-pass IIR of the unwrapped local phase */
/* mm_params.edge_mode: sampler wrap of the engine resamples and the blur
 * (unpinned by the reference) */
#define MM_EDGE_REPEAT 0
#define MM_EDGE_CLAMP  1

/* mm_process flags */
#define MM_FRAMES_ON_DEVICE 1  /* in/out are device pointers (else host memory) */

typedef struct mm_handle mm_handle;

/* Inspector fields of the reference component (.cs:12-43). */
typedef struct {
    int   levels;              /* pyramidLevels            .cs:19  (1..16)      */
    float min_freq;            /* minFrequency             .cs:20               */
    float max_freq;            /* maxFrequency             .cs:21               */
    float phase_scale;         /* phaseScale (PhaseScale)  .cs:29               */
    float magnitude_threshold; /* magnitudeThreshold=0.01  .cs:30               */
    int   orientations;        /* 1 (reference semantics); 4, 6, 8 with MM_MODE_STEERABLE */
    int   mode;                /* MM_MODE_PYRAMID | MM_MODE_STANDARD | MM_MODE_STEERABLE */
    int   edge_mode;           /* MM_EDGE_REPEAT | MM_EDGE_CLAMP                */
    int   apply_magnification; /* applyMotionMagnification .cs:12 (0: passthrough) */
    /* standard mode's phase-delta band-pass (PhaseDifferenceComputeShader.compute:88-122) */
    int   apply_bandpass_filter;  /* applyBandpassFilter  .cs:35 */
    float low_frequency_cutoff;   /* lowFrequencyCutoff   .cs:36 */
    float high_frequency_cutoff;  /* highFrequencyCutoff  .cs:37 */
    float filter_steepness;       /* filterSteepness      .cs:38 */
    float motion_sensitivity;     /* motionSensitivity    .cs:41 */
    int   enhance_edges;          /* enhanceEdges         .cs:42 */
    float edge_enhancement;       /* edgeEnhancement      .cs:43 (used iff enhance_edges, .cs:504) */
    /* debug views (ProcessDebugView .cs:234-257): while either is set the output
     * is the |spectrum| (log-scaled) and/or |phase| view, R channel only (RFloat
     * textures), cropped (one view) or split screen (both); the state still
     * follows the input (.cs:122).  Since ABI 3. */
    int   show_magnitude;         /* showMagnitude        .cs:13 */
    int   show_phase;             /* showPhase            .cs:14 */
    /* MM_MODE_STEERABLE (extension; spec oracle/steerable_ref.py;
     * no reference counterpart): `orientations` in {4, 6, 8} oriented cos^4
     * subbands per middle level, local phase filtered per coefficient by
     * `temporal_filter` (MM_FILTER_DIFF | MM_FILTER_IIR with first-order
     * low-pass coefficients iir_low < iir_high in (0, 1]), amplified by
     * phase_scale; magnitude_threshold gates |subband| < tau.  Since ABI 4. */
    int   temporal_filter;
    float iir_low;
    float iir_high;
} mm_params;

/* Reference defaults (.cs:12-43): levels 5, 0.05/0.45, phaseScale 10, threshold
 * 0.01, pyramid mode; band-pass on, 0.05/0.4, steepness 3, sensitivity 1.5,
 * edges on at 0.8. */
int mm_params_default(mm_params *p);

/* Start()/InitializeProcessor (.cs:90-94, :289-342): geometry frozen here. */
int mm_create(int width, int height, const mm_params *p, int hip_device,
              mm_handle **out);

/* OnValidate (.cs:78-88): new parameters apply from the next frame.  Does not
 * synchronise the device: a change of edge_mode (which rewrites the resample
 * tables) waits only for this handle's own latest work.
 * edge_mode mid-stream: the state is the previous frame's RESAMPLED rows
 * (G_{t-1}, built with the tables of the call that processed that frame), so
 * the first frame after an edge_mode change pairs an old-edge G_{t-1} with a
 * new-edge G_t; from the frame after it both use the new tables.  The
 * reference re-resamples previousSourceTexture with the current sampler every
 * frame (.cs:151); its sampler wrap is an unpinned engine choice (SURVEY.md
 * §8c).  A caller that needs the reference's behaviour exactly calls
 * mm_reset with the change (that frame then passes through). */
int mm_set_params(mm_handle *h, const mm_params *p);
int mm_get_params(const mm_handle *h, mm_params *p);

/* Padded FFT size N (.cs:300-302). */
int mm_padded_size(const mm_handle *h, int *n);

/* Bytes of one W x H frame of `format` (MM_ERR_INVALID for an unknown format
 * or size; MM_ERR_UNSUPPORTED for an NV12 or P010 format with odd W or H).  Since
 * ABI 10. */
int mm_frame_bytes(int width, int height, int format, size_t *bytes);

/* Pitched surfaces (backward-compatible addition to ABI 10: a caller detects it
 * by the presence of mm_surface_bytes).  Frames as a decoder, an encoder or an
 * engine really stores them: rows padded to a pitch, the 4:2:0 (Cb, Cr) plane
 * at an offset of its own (a VCN / VA-API 1080p NV12 surface: pitch 2048, luma
 * padded to 1088 rows), frames of a stream a stride apart; a region of interest
 * inside a larger frame is such a view too (base = its first sample, pitch =
 * the parent's).  Every format, mode and entry point, the input and the output
 * side independently, no repack.
 *   - A pitched frame IS the tight frame of its W x H samples: padding (row
 *     tails, the gap between the planes and between frames, anything past the
 *     last row's W samples) is never read and never written.  The first frame
 *     and apply_magnification = 0 pass the W x H samples through bitwise and
 *     leave the destination's padding alone.
 *   - in_layout and out_layout may differ (decoder surface in, encoder surface
 *     out); their `format` must be equal (MM_ERR_INVALID).
 *   - The temporal state G_{t-1} does not depend on any layout: consecutive
 *     calls of one handle may use different layouts.
 *   - mm_process / mm_process_stream / mm_compute_state are these calls with
 *     mm_surface_tight on both sides: one code path, one set of kernels.
 *     Everything else (debug views, modes, odd sizes of the RGBA formats, edge
 *     modes, host-memory frames, stream ordering, aliasing) follows them.
 * Validation (mm_surface_bytes; every frame entry point applies it before it
 * queues anything; no GPU needed).  With the unit u = the pixel size of an RGBA
 * format (4, 16, 8, 4; MM_BGRA8 / MM_BGRA8_SRGB: 4, and every rule of
 * MM_RGBA8's), 2 for NV12 (a (Cb, Cr) pair), 4 for P010 and packed
 * 4:2:2, 8 for MM_Y210 (a macropixel each) and the sample
 * size of a single-plane format (1 for MM_Y8, 2 for MM_Y10 / Y12 / Y16), 1 for
 * packed RGB (MM_RGB24 / MM_BGR24: any byte):
 *   - unknown format: MM_ERR_INVALID; 4:2:0 with odd W or H: MM_ERR_UNSUPPORTED;
 *   - pitch (4:2:0: and chroma_pitch) at least the row's sample bytes (W pixels;
 *     4:2:0: W samples) and a multiple of u; chroma_offset a multiple of u and
 *     at or past the end of the last luma row's samples; RGBA and single-plane
 *     formats: chroma_offset = chroma_pitch = 0; else MM_ERR_INVALID;
 *   - extent = the byte after the last sample of the last row of the last
 *     plane (not pitch * H: a region of interest at the bottom of its parent
 *     is valid).  The kernels address a frame with 32-bit byte offsets from
 *     its base, so extent <= 2^32 (4 GiB per frame), else MM_ERR_UNSUPPORTED;
 *     an overflow of size_t: MM_ERR_INVALID;
 *   - device frame pointers are aligned to u (MM_ERR_INVALID; host-memory
 *     frames are staged and need no alignment).  (The tight NV12 layout
 *     puts odd frames of a 98 x 62 stream at 2 mod 4, so NV12 asks for the
 *     pair's 2 bytes; 4-byte aligned NV12 surfaces with pitches that are
 *     multiples of 4 get the dword accesses.)  With count > 1, frame_stride is
 *     at least extent and a multiple of u.
 * Wide accesses (RGBA8's 16-byte quads, NV12's dword quads, P010's 8-byte
 * quads; MM_Y210's 16-byte quads are one access at any 8-byte-aligned address)
 * are decided per frame from base, pitch and chroma offset and pitch;
 * an unaligned frame takes the narrower access, never another kernel: a layout
 * aligned like a decoder's runs exactly the tight layout's kernels. */
typedef struct {
    /* MM_I420(_FULL) and MM_I010(_FULL) too: every format of the list above */
    int    format;         /* MM_RGBA8 ... MM_UYVY_FULL, MM_Y210(_FULL), MM_RGB24 / MM_BGR24, MM_BGRA8(_SRGB); 4:2:0 and 4:2:2: | MM_MATRIX_* */
    size_t pitch;          /* bytes from one row to the next: RGBA rows, or luma rows */
    size_t chroma_offset;  /* 4:2:0: bytes from the frame's base to the (Cb,Cr) plane; else 0 */
    size_t chroma_pitch;   /* 4:2:0: bytes from one (Cb,Cr) row to the next; else 0 */
    size_t frame_stride;   /* streams: bytes from frame k to frame k+1 (ignored for one frame) */
} mm_surface;

/* The packed layout of mm_frame_bytes (pitch = row bytes, the chroma plane
 * right after row H - 1, frame_stride = mm_frame_bytes). */
int mm_surface_tight(int width, int height, int format, mm_surface *s);
/* pitch = row bytes rounded up to pitch_align (a multiple of u, >= 1),
 * chroma_pitch = pitch, chroma_offset = pitch x (H rounded up to rows_align;
 * even for 4:2:0), frame_stride = the whole padded planes (4:2:0: pitch x 3/2
 * of the padded rows).  (256, 16) is a hardware decoder's layout: 1080p NV12
 * gives pitch 2048, chroma_offset 2048 x 1088, frame_stride 2048 x 1632. */
int mm_surface_aligned(int width, int height, int format, size_t pitch_align, int rows_align,
                       mm_surface *s);
/* Validates a layout for W x H frames (rules above) and returns its extent. */
int mm_surface_bytes(int width, int height, const mm_surface *s, size_t *extent);

/* OnRenderImage (.cs:101-143): one frame in, one frame out.
 * flags & MM_FRAMES_ON_DEVICE: in/out are device pointers and the call is
 * asynchronous on `hip_stream` (NULL = the default stream, as everywhere in
 * HIP; mm_stream(h) is a non-blocking stream owned by the handle); otherwise
 * in/out are host pointers and the call returns when out is written.
 * Every device-pointer entry point below orders its work on `hip_stream` the
 * same way: a caller that produced the input on another stream synchronises.
 * A call on a different stream than the handle's previous call first makes
 * that stream wait for the previous call's work (since ABI 9: calls of one
 * handle never overlap, whatever streams they use). */
int mm_process(mm_handle *h, const void *in, void *out, int format, int flags,
               void *hip_stream);

/* Consecutive frames of one stream in a single call (device pointers;
 * frame k at in + k * mm_frame_bytes).  Equivalent, frame for frame, to `count`
 * mm_process calls; batches the launches. Asynchronous on hip_stream. */
int mm_process_stream(mm_handle *h, const void *in, void *out, int count,
                      int format, void *hip_stream);

/* mm_process / mm_process_stream on pitched surfaces (see mm_surface). */
int mm_process_surface(mm_handle *h, const void *in, const mm_surface *in_layout,
                       void *out, const mm_surface *out_layout, int flags, void *hip_stream);
int mm_process_stream_surfaces(mm_handle *h, const void *in, const mm_surface *in_layout,
                               void *out, const mm_surface *out_layout, int count, void *hip_stream);

/* ---- Different formats in and out ----------------------------------------
 * (a backward-compatible addition to ABI 10; detect it by the presence of
 * mm_convert_supported)
 * mm_process_surface / mm_process_stream_surfaces keep refusing differing
 * formats with MM_ERR_INVALID.  mm_process_convert / mm_process_stream_convert
 * are those two calls with in_layout->format != out_layout->format allowed for
 * these pairs, every range and matrix variant (the matrix bit belongs to the
 * Y'CbCr side):
 *   decode: any MM_NV12 code (16, 17, 48, 49, 80, 81) or MM_P010 code (18, 19,
 *           50, 51, 82, 83) in, MM_RGBA8 out;
 *   encode: MM_RGBA8 in, any MM_NV12 code out;
 *   and both with MM_BGRA8 in MM_RGBA8's place ("BGRA frames"): the output of
 *   a decode is the MM_RGBA8 decode's with bytes 0 and 2 of every pixel
 *   exchanged, an encode's is the MM_RGBA8 encode's on the exchanged frame.
 * With equal formats they ARE the existing calls: same bytes, same state, same
 * kernels.  mm_convert_supported(in, out) needs no GPU: MM_OK for the pairs
 * above and any valid equal pair, MM_ERR_UNSUPPORTED for every other pair of
 * two valid codes, MM_ERR_INVALID if either code is unknown.
 * Semantics: the frame IS the RGBA32F frame given by the in format's "in"
 * rule, the result is the reference's result on that frame, and it is stored
 * by the out format's "out" rule: MM_RGBA8 round(saturate(v) * 255), alpha
 * 255; NV12 Y', Cb', Cr' of the saturated RGB by the OUT code's weights and
 * range, chroma the mean of the 2 x 2 block, floor(v + 0.5) clamped.  MM_RGBA8
 * to NV12 ignores the input alpha.  P010 to MM_RGBA8 keeps all 16 bits of the
 * words on the input side and rounds once, at the store.  The frame never
 * takes a second trip through memory: the compose stage reads the one format
 * and stores the other.
 * The first frame after mm_create / mm_reset and apply_magnification = 0:
 * there is NO bitwise passthrough between different formats.  The output is
 * the plain conversion: the out rule applied to the in frame's RGBA32F frame,
 * saturated first (one kernel for the n frames, the decode by the format's
 * matrix in fp32).  The destination's padding is untouched.
 * Temporal state: after a convert call it is bitwise the state the same-format
 * call on the in format leaves behind (K1's output, which has no out side).
 * So convert calls, same-format calls and different layouts may alternate on
 * one handle, and mm_get_state / mm_set_state / mm_compute_state* are unchanged.
 * Restrictions are the union of both formats': W and H even, show_magnitude /
 * show_phase refused, both MM_ERR_UNSUPPORTED.  Each layout is validated by its
 * own format's rules (unit, pitch, chroma offset, extent, alignment of device
 * pointers); unknown codes, null pointers and count < 0 are MM_ERR_INVALID; all
 * of it before anything is queued: the handle stays usable and its state is
 * unchanged.  Host-memory frames (flags without MM_FRAMES_ON_DEVICE) are
 * staged per side with each side's own frame size; the stream form takes
 * device pointers only and is equivalent, frame for frame, to `count` single
 * calls.  Every mode, both edge modes and every batch size work.
 * The fused kernels run where each side's quads are aligned: NV12 in, the
 * input's chroma rows on multiples of 4 bytes; MM_RGBA8 in with NV12 out, the
 * output's luma and chroma rows; the MM_RGBA8 and P010 sides in every layout.
 * Any other legal layout takes the unfused kernels: the same bytes.
 * Out of scope: any pair not listed (packed 4:2:2 or MM_Y210 to MM_RGBA8,
 * MM_RGBA8 to P010, P010 to MM_RGBA16F, MM_RGB24 / MM_BGR24 on either side of a
 * mixed pair, MM_RGB24 to MM_BGR24 included, MM_RGBA8 to MM_BGRA8,
 * MM_RGBA8_SRGB and MM_BGRA8_SRGB, grayscale, Y'CbCr
 * to Y'CbCr transcodes such as NV12 to P010 or a matrix change); scaling or
 * cropping between the sides; chroma siting other than the shared 2 x 2
 * sample; PQ / HLG; odd sizes; the debug views; the ring entry points
 * (include/mm_ring.h); the Unity shim; mm_extmem_check. */
int mm_convert_supported(int in_format, int out_format);
int mm_process_convert(mm_handle *h, const void *in, const mm_surface *in_layout,
                       void *out, const mm_surface *out_layout, int flags, void *hip_stream);
int mm_process_stream_convert(mm_handle *h, const void *in, const mm_surface *in_layout,
                              void *out, const mm_surface *out_layout, int count, void *hip_stream);

/* isFirstFrame = true (.cs:75): the next frame is passed through.  The same
 * happens after a MM_MODE_STEERABLE mm_set_state followed by a switch to
 * another mode (that state holds local phases, not G_{t-1}). */
int mm_reset(mm_handle *h);

/* The temporal state carried between frames (previousSourceTexture, .cs:142):
 * the previous input frame's row half-spectra G_{t-1} (K1's output: complex
 * fp32 [N/2 + 1][H rounded up to even], rows of the windowed luma after the
 * stretch+pad resample; 8.86 MB at 1920x1080), from which the next call
 * recomputes the previous frame's 2D spectrum.  `dev_buf` is device memory of
 * mm_state_size() bytes.  Ordered on hip_stream (NULL = default stream).
 * MM_MODE_STEERABLE: the per-coefficient local phases (one float plane per
 * band; MM_FILTER_IIR adds the two filter planes), so the size follows the
 * mode, levels, orientations and filter of the current parameters. */
int mm_state_size(const mm_handle *h, size_t *bytes);
int mm_get_state(mm_handle *h, void *dev_buf, size_t bytes, void *hip_stream);
int mm_set_state(mm_handle *h, const void *dev_buf, size_t bytes, void *hip_stream);
/* Compute the state that frame `in` would leave behind (its row spectra) into
 * dev_buf without touching the handle's own state (used by the multi-GPU ring
 * to hand the chunk-boundary state to the next rank). */
int mm_compute_state(mm_handle *h, const void *in_dev, int format, void *dev_buf,
                     size_t bytes, void *hip_stream);
int mm_compute_state_surface(mm_handle *h, const void *in_dev, const mm_surface *in_layout,
                             void *dev_buf, size_t bytes, void *hip_stream);

/* The handle's HIP stream (hipStream_t). */
void *mm_stream(mm_handle *h);

/* Frames per internal batch of mm_process_stream: the launches of one batch
 * cover `frames` frames, and the column kernel keeps the previous spectrum on
 * chip across them (each launch first re-transforms the state G_{t-1}).
 * Larger batches amortise that and the launch gaps; the hand-off buffers take
 * about 17.8 MB per 1080p frame (4x at 2160p).  Default: min(64, 2 GiB of
 * buffers).  Results do not depend on the batch size.  MM_MODE_STEERABLE
 * holds, besides, the band rows of one column chunk independent of the batch
 * (O = 8: 231 MB per 1080p frame x 8 frames, 1.2 GB per 2160p frame x 2; the
 * MM_SB_CF environment variable, 2..16, sets the 1080p chunk) and the state
 * planes (100 MB DIFF / 300 MB IIR at 1080p).  Reallocates: the
 * old buffers retire behind this handle's latest work and the call waits for
 * that work only (not for the device, since ABI 9); call between frames.
 * Failure-atomic: on MM_ERR_OOM the handle keeps its previous batch size,
 * buffers and state.  Since ABI 5. */
int mm_set_batch(mm_handle *h, int frames);
int mm_get_batch(const mm_handle *h, int *frames);

/* ---- Several live streams in one call -------------------------------------
 * (a backward-compatible addition to ABI 10; detect it by the presence of
 * mm_set_lanes)
 * mm_process_stream batches consecutive frames of ONE stream, which a live
 * source never has: a camera hands over one frame per tick.  A rig of M
 * cameras of one geometry batches over the cameras instead: output t of a
 * stream depends only on frames t-1 and t of that stream, so one call advances
 * M streams by one frame each with one launch per kernel.
 * A lane is one stream's temporal state (G_{t-1}), owned by the handle.  All
 * lanes share the handle's geometry and mm_params.  Lane state is separate
 * from the handle's own single-stream state: mm_process*, mm_get_state,
 * mm_set_state, mm_reset, mm_set_batch and the rest behave exactly as before
 * and may be interleaved with lane calls on one handle; neither disturbs the
 * other.
 * mm_set_lanes(h, lanes), 1 .. MM_LANES_MAX, allocates two G slots and one Q
 * slot per lane (about 26.6 MB per 1080p lane: the 17.8 MB of a batch frame
 * plus one more G slot); 0 frees them.  Another count than the current one
 * drops every lane's state; the same count is a no-op.  Failure-atomic like
 * mm_set_batch: on MM_ERR_OOM the previous lanes and their state stay.  The old
 * buffers retire behind this handle's own work, never the device's; call it
 * between frames.  mm_destroy releases the lanes.
 * mm_process_lanes advances EVERY lane by one frame: frame k of the call is
 * lane k's next frame, at in + k * in_layout->frame_stride, its output at
 * out + k * out_layout->frame_stride.  Device pointers only; asynchronous on
 * hip_stream and ordered like every other entry point.  The layouts are
 * validated as mm_process_stream_surfaces validates them with count = lanes;
 * the formats are equal or a pair of mm_convert_supported (the state after the
 * call is the in frame's, as for convert calls).
 * The contract is bitwise: lane k's outputs, and its state after every call,
 * are those of a handle of its own with the same parameters, fed lane k's
 * frames through one mm_process_surface / mm_process_convert call each.
 * A lane without state (after mm_set_lanes, mm_reset_lane, or mm_set_lanes to
 * another count) passes its frame through bitwise; for a convert pair that is
 * the plain conversion, as for single calls.  A lane has state after a call or
 * after mm_set_lane_state.  apply_magnification = 0: every frame passes through
 * and every lane's state follows its input.  mm_set_params applies to all lanes
 * from the next call; its edge_mode note holds per lane.
 * mm_reset_lane(h, lane) is mm_reset for one lane; lane = -1: every lane.
 * mm_get_lane_state / mm_set_lane_state move mm_state_size() bytes in
 * mm_get_state's format: a stream moves between a single-stream handle and a
 * lane, or between lanes, and continues bitwise.  (A lane without state:
 * MM_ERR_NO_STATE from mm_get_lane_state.)
 * Refusals, all before anything is queued; the handle and every lane's state
 * stay as they were.  MM_ERR_UNSUPPORTED: MM_MODE_STEERABLE (its state is
 * 100-300 MB per stream), show_magnitude or show_phase, from mm_process_lanes
 * and the two lane-state calls; a handle with N = 8192, from mm_set_lanes; odd
 * sizes of the Y'CbCr formats, as everywhere.  MM_ERR_INVALID: null pointers, a
 * lane index out of range, lanes outside 0 .. MM_LANES_MAX, mm_process_lanes
 * with no lanes set, a `bytes` below mm_state_size(), two different formats that
 * are no supported pair.
 * A subset of the lanes per call (a further backward-compatible addition to
 * ABI 10; detect it by the presence of mm_process_lanes_mask).  Live sources
 * are not genlocked, drop frames and run at different rates, so
 * mm_process_lanes_mask advances only the lanes of `mask`: bit k selects lane
 * k.  The addressing stays lane-indexed whatever the mask, one slot per
 * camera: lane k's frame at in + k * in_layout->frame_stride, its output at
 * out + k * out_layout->frame_stride.  Of a lane that is not selected the
 * input slot is not read, the output slot is not written, and its state, its
 * has-state flag and a pending mm_set_params edge_mode transition are
 * untouched.  The bitwise contract above holds per lane over the frames of the
 * calls that selected it, in order: a handle of its own fed exactly those
 * frames.  Everything mm_process_lanes promises holds per selected lane
 * (passthrough without state, apply_magnification = 0, every format, layout
 * and convert pair, both edge modes, both modes).  A lane call's frames may be
 * processed in place, in == out with one layout on both sides: the compose
 * reads source rows beside the ones it writes, so such a call first copies the
 * frames it composes aside and gives the same bytes as a call with separate
 * buffers.  That is the one case where a handle with lanes holds more than two
 * G slots and a Q slot per lane: one tight frame per lane more (8.3 MB per
 * 1080p RGBA8 lane), allocated at the first such call, before anything is
 * queued (MM_ERR_OOM then leaves the handle and every lane as they were), and
 * one frame copy per composed lane and call; a frame copy, not a state copy.
 * Buffers that overlap in any other way are not supported.  The mask of all
 * lanes IS mm_process_lanes (which is that call): same bytes, same states; the
 * two may alternate on one handle with each other, with the single-stream
 * calls and with the lane-state calls.  mask = 0 returns MM_OK, queues
 * nothing and changes nothing (in and out may then be anything).  The layouts
 * are validated with count = (the highest selected lane) + 1: a buffer need
 * not extend past the last lane the call selects.  mm_lanes_with_state: bit k
 * of *mask is set where lane k has state.  Refusals as above, and
 * MM_ERR_INVALID for a mask bit at or above the lane count.
 * No state is copied, for lanes that advance or for lanes that sit out: each
 * lane has a bank bit of its own, naming the G slot of its two that holds its
 * state; a call writes the other slot and flips the bit of the lanes it
 * selected.  The column kernel runs once per call over any mask.  The row
 * kernels run once per RUN of consecutive selected lanes; a forward run also
 * ends where the bank bits of neighbours differ (after a lane sat out an odd
 * number of calls), a compose run where a lane without state meets one with.
 * So a fragmented mask costs launches, never results: a caller with rate
 * groups (30 and 60 fps sources) orders its lanes by group, so that each
 * group is one run with one bank bit.
 * Out of scope: one row-kernel launch over a mask with holes; lanes of
 * different sizes or parameters; host-memory frames; the ring entry points. */
#define MM_LANES_MAX 64
int mm_set_lanes(mm_handle *h, int lanes);            /* 1..MM_LANES_MAX; 0 frees */
int mm_get_lanes(const mm_handle *h, int *lanes);
int mm_process_lanes(mm_handle *h, const void *in, const mm_surface *in_layout,
                     void *out, const mm_surface *out_layout, void *hip_stream);
int mm_process_lanes_mask(mm_handle *h, uint64_t mask,
                          const void *in, const mm_surface *in_layout,
                          void *out, const mm_surface *out_layout, void *hip_stream);
int mm_lanes_with_state(const mm_handle *h, uint64_t *mask);   /* bit k: lane k has state */
int mm_reset_lane(mm_handle *h, int lane);            /* -1: every lane */
int mm_get_lane_state(mm_handle *h, int lane, void *dev_buf, size_t bytes, void *hip_stream);
int mm_set_lane_state(mm_handle *h, int lane, const void *dev_buf, size_t bytes, void *hip_stream);

/* ---- Held reference frame --------------------------------------------------
 * (a backward-compatible addition to ABI 10; detect it by the presence of
 * mm_set_hold)
 * By default the state is G_{t-1}: it follows the input on every call, and the
 * operator magnifies the phase change between two consecutive frames (the
 * reference's behaviour).  Measuring displacement against a rest frame (a
 * structure against its unloaded picture, a pipe against the frame before the
 * pump started) wants every frame paired with ONE reference frame R instead.
 * mm_set_hold(h, 1) does that, from the next call on:
 * While hold is set, frames do not advance the handle's single-stream state:
 * every frame of every call pairs with the state R the handle had when the
 * call began.  The contract is bitwise: the output of frame x is the output a
 * handle of its own with the same parameters gives for mm_set_state(R)
 * followed by one one-frame call on x, with the same formats and layouts;
 * mm_get_state after the call returns R bit for bit.  It holds in pyramid and
 * standard mode, both edge modes, every size, format, layout and convert pair,
 * for the one-frame, stream, host-memory and lane calls, and for every batch
 * size and batch boundary.  Inside a batch the column kernel transforms R once
 * per workgroup and launch, not once per frame (1080p: a held stream runs at
 * the rolling stream's rate, 2.9 times the mm_set_state-per-frame pattern's).
 * Without state (after mm_create, mm_reset, mm_reset_lane) the first frame
 * passes through, as always, and becomes R; the remaining frames of the same
 * call already pair with it.  mm_reset plus hold therefore means "the next
 * frame is the reference".
 * apply_magnification = 0: every frame passes through.  With state nothing
 * else happens (no kernel but the copy runs; in a lane call, none for the held
 * lanes that have state); without state the first frame of the call becomes R.
 * Switching hold off: the next call behaves as always, its first frame pairs
 * with R and the state follows the input again.  Re-referencing every k frames
 * is therefore "one frame with hold off": no passthrough frame, no further
 * entry point.  mm_set_state, or mm_compute_state plus mm_set_state, installs
 * any frame as the reference.
 * Other calls: mm_set_params applies as always, and its edge_mode note reads
 * "the held R keeps the tables it was built with until the caller
 * re-references".  mm_set_batch keeps R bit for bit.  mm_compute_state* is
 * unaffected.
 * Lanes hold one by one: bit k of mm_set_lanes_hold's mask makes lane k hold.
 * mm_set_lanes to another count clears the mask, the same count keeps it.  A
 * held lane's forward row kernel writes the slot of the bank that does not
 * hold its state, the column kernel reads both, and the lane's bank bit is not
 * flipped: no state is copied and no memory is added.  A held lane without
 * state passes through, gets state and its bank bit as always.  Held and
 * rolling lanes side by side end up with different bank bits every second
 * call, which splits forward runs: it costs launches, never results.  As with
 * rate groups, a caller orders its lanes by hold group.
 * Refusals, all before anything is queued; state and flags stay as they were.
 * With hold set, MM_MODE_STEERABLE and show_magnitude / show_phase give
 * MM_ERR_UNSUPPORTED from every frame entry point (the flag itself may be set
 * in any mode).  MM_ERR_INVALID: null pointers, a hold value other than 0 or
 * 1, a mask bit at or above the lane count.
 * Out of scope: a lag of k frames (k interleaved streams: lanes); a temporal
 * band-pass in pyramid mode; hold in steerable mode and the debug views; the
 * ring entry points. */
int mm_set_hold(mm_handle *h, int hold);              /* 0 | 1, else MM_ERR_INVALID; applies from the next call */
int mm_get_hold(const mm_handle *h, int *hold);
int mm_set_lanes_hold(mm_handle *h, uint64_t mask);   /* bit k: lane k holds; a bit at or above the lane count: MM_ERR_INVALID */
int mm_get_lanes_hold(const mm_handle *h, uint64_t *mask);

/* Zero-copy frames (f4): device memory owned by another API — an engine's
 * render target exported as an opaque POSIX fd (Vulkan VK_KHR_external_memory_fd,
 * or a HIP VMM allocation via hipMemExportToShareableHandle) — imported into the
 * handle's device (hipImportExternalMemory) and mapped as a device pointer that
 * mm_process / mm_process_stream take with MM_FRAMES_ON_DEVICE, in place: no
 * staging copy, no PCIe transfer (the reference's OnRenderImage works on the
 * engine's RenderTextures, .cs:101).  `bytes` = the exported allocation's
 * size, `offset` = where the frames start in it.  On success the fd belongs to
 * the import (do not close it).  Release before the exporter frees the memory.
 * Since ABI 6. */
typedef struct mm_ext_frames mm_ext_frames;
int mm_import_frames(mm_handle *h, int fd, size_t bytes, size_t offset, mm_ext_frames **out);
void *mm_ext_frames_ptr(const mm_ext_frames *x);
int mm_release_frames(mm_ext_frames *x);

/* OnDestroy/ReleaseResources (.cs:96-99, :344-356).  Returns the handle's
 * device memory to the device's stream-ordered pool behind the handle's own
 * latest work (every call that queued work records an event) and waits for
 * that work only, never for the whole device: other handles and streams on
 * the GPU keep running.  Work the CALLER queued on its streams that reads
 * handle-owned memory (none through this API: frames are caller-owned) is the
 * caller's to finish first.  Since ABI 9.
 * Hardware-queue caveat (this and mm_set_params / mm_set_batch): the HIP
 * runtime maps streams onto GPU_MAX_HW_QUEUES hardware queues (default 4)
 * round-robin, and streams that share a hardware queue execute in one order.
 * With more live streams than queues, this handle's stream can sit behind
 * another stream's blocked work on the same queue, and the wait for "this
 * handle's own work" then also waits for that work.  The entry point itself
 * never synchronises the device; a process that must not couple streams that
 * way raises GPU_MAX_HW_QUEUES (tests/test_handle.py runs its no-stall tests
 * with 16). */
void mm_destroy(mm_handle *h);

const char *mm_strerror(int code);
int mm_abi_version(void);

/* ---- utilities (not on the reference surface) ---- */
/* Per-kernel device time, measured with HIP events recorded on the launch
 * stream around every launch between mm_profile_begin and mm_profile_end.
 * Kernel ids: */
#define MM_K_ROWS_FWD 0   /* K1: resample + window + row real FFT      */
#define MM_K_COLS     1   /* K2: column FFT + pyramid phase op + IFFT  */
#define MM_K_ROWS_INV 2   /* K3: row C2R IFFT + |z| + horizontal blur    */
#define MM_K_COMPOSE  3   /* K4: vertical blur + YIQ recombine + RGB + crop */
#define MM_K_ROWS_INV_COMPOSE 4   /* K3 + K4 fused (even sizes, N - H >= 4)  */
#define MM_K_COUNT    5
int mm_profile_begin(mm_handle *h);
/* Waits for the recorded events; ms[k] = summed device ms, launches[k],
 * frames[k] = frames processed by kernel k, k < MM_K_COUNT (arrays of
 * MM_K_COUNT entries; any pointer may be NULL). */
int mm_profile_end(mm_handle *h, double *ms, int *launches, int *frames);

/* Synthetic stream frames generated on the device:
 * frames t0..t0+count-1 into dev_out (RGBA8). */
int mm_synth_frames(void *dev_out, int width, int height, int t0, int count,
                    uint64_t seed, int gray, void *hip_stream);

/* Host-side geometry tables (no GPU needed), exposed for tests:
 * per image column (row) the 4 source indices and 4 weights of the composite
 * stretch+pad bilinear resample, including the Hann window factor. */
int mm_resample_table(int width, int height, int axis, int edge_mode,
                      int32_t *idx4, float *w4);
/* The (cb, cr) -> (I, Q) matrix the NV12 and P010 compose uses, m = {I_cb, Q_cb, I_cr,
 * Q_cr}: RGBToYIQ's I and Q rows times the BT.601 conversion above, derived
 * in double (the kernels take it divided by the range's chroma scale). */
int mm_nv12_chroma_matrix(double m[4]);
/* The (cb, cr) -> (Y, I, Q) matrix of a 4:2:0 or packed 4:2:2 (8- or 10-bit) format, m = {Y_cb, I_cb, Q_cb,
 * Y_cr, I_cr, Q_cr}: RGBToYIQ's rows times the format's decode (its matrix
 * bit's; the range does not enter), derived in double.  Y_cb, Y_cr are the a,
 * b of Yq above; for the BT.601 codes they are exactly 0 and the I, Q entries
 * mm_nv12_chroma_matrix's.  MM_ERR_INVALID for any other format. */
int mm_ycbcr_matrix(int format, double m[6]);

#ifdef __cplusplus
}
#endif
#endif
