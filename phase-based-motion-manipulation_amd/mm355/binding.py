"""ctypes binding of include/mm.h (lib/libmm355.so)."""
import ctypes
import os
import re

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPO_ROOT = os.path.dirname(PKG_DIR)
LIB_PATH = os.path.join(PKG_DIR, "lib", "libmm355.so")
HEADER = os.path.join(REPO_ROOT, "include", "mm.h")

RGBA8 = 0
RGBA32F = 1
RGBA16F = 2         # linear half (the reference camera's HDR target), ABI 10
RGBA8_SRGB = 3      # 8-bit sRGB target in Linear colour space, ABI 10
# grayscale camera frames, one plane: H rows of W bytes (Y8) or of W
# little-endian 16-bit words with the code in the LOW bits (GenICam Mono8 /
# Mono10 / Mono12 / Mono16); every size, mode and debug view
Y8 = 8              # v = byte / 255
Y10 = 9             # v = word / 1023
Y12 = 10            # v = word / 4095
Y16 = 11            # v = word / 65535
MONO_FORMATS = (Y8, Y10, Y12, Y16)
MONO_BITS = {Y8: 8, Y10: 10, Y12: 12, Y16: 16}
# packed 8-bit Y'CbCr 4:2:2 capture frames, one plane: H rows of W/2 four-byte
# macropixels (W and H even); a matrix bit may be OR-ed on as on the 4:2:0 codes
YUY2 = 24           # bytes Y0 Cb Y1 Cr, BT.601 limited range
YUY2_FULL = 25      # full range
UYVY = 26           # bytes Cb Y0 Cr Y1, BT.601 limited range
UYVY_FULL = 27      # full range
PACKED422_FORMATS = (YUY2, YUY2_FULL, UYVY, UYVY_FULL)
# 10-bit packed 4:2:2, one plane: H rows of W/2 eight-byte macropixels, four
# little-endian 16-bit words Y0 Cb Y1 Cr, each the 10-bit code << 6 as in P010 (a
# Y216 surface's low bits are honoured); W and H even; a matrix bit may be OR-ed on
Y210 = 22           # BT.601 limited range
Y210_FULL = 23      # full range
Y210_FORMATS = (Y210, Y210_FULL)
# packed RGB, what cv2 / PIL / imageio / torchvision / ffmpeg rgb24, bgr24 / PPM
# hand out: [H, W, 3] bytes, no alpha; every size, mode and debug view.  The
# byte-order bit is valid on RGB24 alone (the B G R A orders are formats of their
# own with a bit of their own, ORDER_BGRA below).
RGB24 = 13          # bytes R G B, v = byte / 255 as RGBA8
ORDER_BGR = 128     # byte-order bit: B G R (OpenCV's order)
BGR24 = RGB24 | ORDER_BGR
RGB24_FORMATS = (RGB24, BGR24)
# B G R A, what D3D / Vulkan swap chains, DXGI desktop duplication, CoreVideo (32BGRA),
# NDI, DeckLink's 8-bit BGRA mode, Qt, Cairo and OpenCV's four-channel mats hand out:
# [H, W, 4] bytes, the RGBA8 (RGBA8_SRGB) frame with bytes 0 and 2 of every pixel
# exchanged; every size, mode and debug view.  The bit is valid on those two codes alone.
ORDER_BGRA = 8192   # byte-order bit of the 4-byte UNORM formats: B G R A
BGRA8 = RGBA8 | ORDER_BGRA              # 8192
BGRA8_SRGB = RGBA8_SRGB | ORDER_BGRA    # 8195
BGRA_FORMATS = (BGRA8, BGRA8_SRGB)
FORMAT_BPP = {RGBA8: 4, RGBA32F: 16, RGBA16F: 8, RGBA8_SRGB: 4, Y8: 1, Y10: 2, Y12: 2, Y16: 2,
              YUY2: 2, YUY2_FULL: 2, UYVY: 2, UYVY_FULL: 2, Y210: 4, Y210_FULL: 4, RGB24: 3, BGR24: 3,
              BGRA8: 4, BGRA8_SRGB: 4}
# video frames, planar 8-bit Y'CbCr 4:2:0 (H rows of W luma bytes, then H/2 rows
# of W interleaved Cb, Cr bytes; W and H even): frame_bytes() gives W*H*3/2
NV12 = 16           # BT.601 limited ("video") range
NV12_FULL = 17      # full ("JPEG") range
# 10-bit video frames, the same layout in little-endian 16-bit words (10-bit code
# << 6; a P016 surface's low bits are honoured): frame_bytes() gives W*H*3
P010 = 18           # BT.601 matrix, limited range (Y 64..940, C 64..960)
P010_FULL = 19      # full range (0..1023)
# three-plane 8-bit 4:2:0 (I420, ffmpeg's yuv420p, a C420 .y4m's frames): H rows of
# W luma bytes, then H/2 rows of W/2 Cb bytes, then H/2 rows of W/2 Cr bytes, NV12's
# samples and semantics; the plane-layout bit is valid on the two NV12 codes alone
PLANAR = 512        # plane-layout bit: Cb and Cr in planes of their own
I420 = NV12 | PLANAR            # 528, BT.601 limited range
I420_FULL = NV12_FULL | PLANAR  # 529, full range
I420_FORMATS = (I420, I420_FULL)
# 10-bit three-plane 4:2:0 (I010, ffmpeg's yuv420p10le, a C420p10 .y4m's frames): the
# same three planes in little-endian 16-bit words with the code in the word's LOW 10
# bits, P010's codes and semantics; frame_bytes() gives W*H*3.  The low-bits bit is
# valid only together with the plane bit on the two P010 codes
LOW_BITS = 1024     # word-alignment bit: the code in the word's low bits
I010 = P010 | PLANAR | LOW_BITS            # 1554, BT.601 limited range
I010_FULL = P010_FULL | PLANAR | LOW_BITS  # 1555, full range
I010_FORMATS = (I010, I010_FULL)
# v210 capture frames (SDI / HDMI cards' 10-bit mode, ffmpeg's v210): Y210's samples,
# three 10-bit codes to a little-endian dword and six pixels to a group of four
# dwords; rows of row_bytes() in the pitch every SDK uses, 128 * ceil(W / 48).  The
# pack bit is valid on the two Y210 codes alone, with or without one matrix bit.
PACK_V210 = 4096    # packing bit: three 10-bit codes per dword
V210 = Y210 | PACK_V210            # 4118, BT.601 limited range
V210_FULL = Y210_FULL | PACK_V210  # 4119, full range
V210_FORMATS = (V210, V210_FULL)
# the grouped formats (no bytes per pixel, so no FORMAT_BPP entry): pixels and bytes
# of a group, and what the tight frame's pitch is a multiple of
FORMAT_GROUP = {V210: (6, 16, 128), V210_FULL: (6, 16, 128)}


def row_bytes(width, fmt):
    """Bytes of the samples of one row (of the first plane) of a FORMAT_BPP or
    FORMAT_GROUP format.  A grouped format's partial last group takes the whole
    dwords its pixels need: v210 rows are 4 * (4 * (W // 6) + (0, 2, 3)[W % 6 // 2])."""
    base = base_format(fmt)
    if base in FORMAT_GROUP:
        px, nbytes, _ = FORMAT_GROUP[base]
        rem = width % px
        return width // px * nbytes + 4 * ((rem * nbytes + 4 * px - 1) // (4 * px))
    return width * FORMAT_BPP[base]


def tight_pitch(width, fmt):
    """The row pitch of Surface.tight / frame_bytes: row_bytes, rounded up to the
    grouped format's pitch multiple (v210: 128 * ceil(W / 48))."""
    rb = row_bytes(width, fmt)
    align = FORMAT_GROUP.get(base_format(fmt), (0, 0, 1))[2]
    return (rb + align - 1) // align * align


# one matrix bit, OR-ed onto a 4:2:0 or packed 4:2:2 code above (HD / UHD content): the layout
# and sizes stay the base code's (base_format)
MATRIX_BT709 = 32   # Kr 0.2126, Kb 0.0722
MATRIX_BT2020 = 64  # Kr 0.2627, Kb 0.0593, non-constant luminance
EDGE_REPEAT = 0
EDGE_CLAMP = 1
MODE_PYRAMID = 0
MODE_STANDARD = 1
MODE_STEERABLE = 2      # extension f2 (oracle/steerable_ref.py)
FILTER_DIFF = 0
FILTER_IIR = 1
FRAMES_ON_DEVICE = 1

KERNELS = ("k_rows_fwd", "k_cols", "k_rows_inv", "k_compose",
           "k_rows_inv_compose")   # MM_K_* ids 0..4

ERRORS = {0: "MM_OK", -1: "MM_ERR_INVALID", -2: "MM_ERR_UNSUPPORTED", -3: "MM_ERR_HIP",
          -4: "MM_ERR_NO_DEVICE", -5: "MM_ERR_OOM", -6: "MM_ERR_NO_STATE"}


class MMError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = code
        name = ERRORS.get(code, str(code))
        super().__init__(f"{what}: {name} ({strerror(code) if _lib else ''})")


class Params(ctypes.Structure):
    """mm_params — the inspector fields of the reference (.cs:12-31)."""
    _fields_ = [("levels", ctypes.c_int), ("min_freq", ctypes.c_float),
                ("max_freq", ctypes.c_float), ("phase_scale", ctypes.c_float),
                ("magnitude_threshold", ctypes.c_float), ("orientations", ctypes.c_int),
                ("mode", ctypes.c_int), ("edge_mode", ctypes.c_int),
                ("apply_magnification", ctypes.c_int),
                ("apply_bandpass_filter", ctypes.c_int), ("low_frequency_cutoff", ctypes.c_float),
                ("high_frequency_cutoff", ctypes.c_float), ("filter_steepness", ctypes.c_float),
                ("motion_sensitivity", ctypes.c_float), ("enhance_edges", ctypes.c_int),
                ("edge_enhancement", ctypes.c_float),
                ("show_magnitude", ctypes.c_int), ("show_phase", ctypes.c_int),
                ("temporal_filter", ctypes.c_int), ("iir_low", ctypes.c_float),
                ("iir_high", ctypes.c_float)]

    @classmethod
    def make(cls, levels=5, min_freq=0.05, max_freq=0.45, phase_scale=10.0,
             magnitude_threshold=0.01, edge_mode=EDGE_REPEAT, apply_magnification=True,
             mode=MODE_PYRAMID, **standard):
        """other mm.h fields by keyword: the standard-mode band-pass
        (apply_bandpass_filter, low_frequency_cutoff, high_frequency_cutoff,
        filter_steepness, motion_sensitivity, enhance_edges, edge_enhancement)
        the debug views (show_magnitude, show_phase) and the steerable
        extension (orientations, temporal_filter, iir_low, iir_high)."""
        p = cls()
        lib().mm_params_default(ctypes.byref(p))
        p.levels, p.min_freq, p.max_freq = levels, min_freq, max_freq
        p.phase_scale, p.magnitude_threshold = phase_scale, magnitude_threshold
        p.edge_mode, p.apply_magnification = edge_mode, 1 if apply_magnification else 0
        p.mode = mode
        for k, v in standard.items():
            if k not in dict(cls._fields_):
                raise TypeError(f"unknown mm_params field {k}")
            setattr(p, k, int(v) if k in ("apply_bandpass_filter", "enhance_edges",
                                          "show_magnitude", "show_phase", "orientations",
                                          "temporal_filter") else v)
        return p


class Surface(ctypes.Structure):
    """mm_surface — where the frames of one side of a call lie: row pitch, the
    4:2:0 (Cb, Cr) plane's offset and pitch, the stride between the frames of a
    stream, all in bytes (include/mm.h)."""
    _fields_ = [("format", ctypes.c_int), ("pitch", ctypes.c_size_t),
                ("chroma_offset", ctypes.c_size_t), ("chroma_pitch", ctypes.c_size_t),
                ("frame_stride", ctypes.c_size_t)]

    @classmethod
    def tight(cls, width, height, fmt):
        """mm_surface_tight: the packed layout of frame_bytes()."""
        s = cls()
        check(_surface_fn("mm_surface_tight")(width, height, fmt, ctypes.byref(s)), "mm_surface_tight")
        return s

    @classmethod
    def aligned(cls, width, height, fmt, pitch_align=256, rows_align=16):
        """mm_surface_aligned: pitch rounded up to pitch_align, planes padded to
        rows_align rows ((256, 16): a hardware decoder's surface)."""
        s = cls()
        check(_surface_fn("mm_surface_aligned")(width, height, fmt, pitch_align, rows_align,
                                                ctypes.byref(s)), "mm_surface_aligned")
        return s

    def bytes(self, width, height):
        """mm_surface_bytes: validates the layout for W x H frames; the byte
        after the last sample of the last row of the last plane."""
        n = ctypes.c_size_t()
        check(_surface_fn("mm_surface_bytes")(width, height, ctypes.byref(self), ctypes.byref(n)),
              "mm_surface_bytes")
        return n.value

    def __repr__(self):
        return (f"Surface(format={self.format}, pitch={self.pitch}, chroma_offset={self.chroma_offset}, "
                f"chroma_pitch={self.chroma_pitch}, frame_stride={self.frame_stride})")


SURFACE_SYMBOLS = ("mm_surface_tight", "mm_surface_aligned", "mm_surface_bytes", "mm_process_surface",
                   "mm_process_stream_surfaces", "mm_compute_state_surface")


def has_surfaces():
    """The loaded library takes pitched surfaces (detected, as include/mm.h
    says, by the presence of mm_surface_bytes)."""
    return hasattr(lib(), "mm_surface_bytes")


def _surface_fn(name):
    if not has_surfaces():
        raise MMError(-2, f"{library_path()} has no {name} (a build from before the pitched surfaces)")
    return getattr(lib(), name)


# different formats in and out (include/mm.h "Different formats in and out"):
# NV12 / P010 codes in with RGBA8 or BGRA8 out, RGBA8 or BGRA8 in with an NV12 code out
CONVERT_SYMBOLS = ("mm_convert_supported", "mm_process_convert", "mm_process_stream_convert")


def has_convert():
    """The loaded library converts between formats (detected, as include/mm.h
    says, by the presence of mm_convert_supported)."""
    return hasattr(lib(), "mm_convert_supported")


def _convert_fn(name):
    if not has_convert():
        raise MMError(-2, f"{library_path()} has no {name} (a build from before the format conversion)")
    return getattr(lib(), name)


def convert_supported(in_fmt, out_fmt):
    """mm_convert_supported: 0 (MM_OK) where frames of in_fmt can come out as
    out_fmt, -2 (MM_ERR_UNSUPPORTED) for any other pair of valid codes, -1
    (MM_ERR_INVALID) if either code is unknown.  Needs no GPU."""
    return _convert_fn("mm_convert_supported")(int(in_fmt), int(out_fmt))


def has_bgra():
    """The loaded library takes B G R A frames (detected, as include/mm.h says, by
    mm_frame_bytes(W, H, MM_BGRA8, &n) == MM_OK).  Needs no GPU."""
    n = ctypes.c_size_t()
    return lib().mm_frame_bytes(2, 2, BGRA8, ctypes.byref(n)) == 0


# several live streams in one call (include/mm.h "Several live streams in one
# call"): one frame of each of a handle's lanes per mm_process_lanes
LANES_SYMBOLS = ("mm_set_lanes", "mm_get_lanes", "mm_process_lanes", "mm_reset_lane",
                 "mm_get_lane_state", "mm_set_lane_state")
LANES_MAX = 64      # MM_LANES_MAX


def has_lanes():
    """The loaded library runs lanes (detected, as include/mm.h says, by the
    presence of mm_set_lanes)."""
    return hasattr(lib(), "mm_set_lanes")


def _lanes_fn(name):
    if not has_lanes():
        raise MMError(-2, f"{library_path()} has no {name} (a build from before the lanes)")
    return getattr(lib(), name)


# a subset of the lanes per call (a later addition: a tuple of its own, so that
# a library from before it still loads and has_lanes() still answers for it)
LANES_MASK_SYMBOLS = ("mm_process_lanes_mask", "mm_lanes_with_state")


def has_lanes_mask():
    """The loaded library advances a subset of the lanes per call (detected, as
    include/mm.h says, by the presence of mm_process_lanes_mask)."""
    return hasattr(lib(), "mm_process_lanes_mask")


def _lanes_mask_fn(name):
    if not has_lanes_mask():
        raise MMError(-2, f"{library_path()} has no {name} (a build from before the lane masks)")
    return getattr(lib(), name)


# a held reference frame (include/mm.h "Held reference frame"): frames pair with
# the state and do not advance it
HOLD_SYMBOLS = ("mm_set_hold", "mm_get_hold", "mm_set_lanes_hold", "mm_get_lanes_hold")


def has_hold():
    """The loaded library holds a reference frame (detected, as include/mm.h
    says, by the presence of mm_set_hold)."""
    return hasattr(lib(), "mm_set_hold")


def _hold_fn(name):
    if not has_hold():
        raise MMError(-2, f"{library_path()} has no {name} (a build from before the held reference)")
    return getattr(lib(), name)


_lib = None
_lib_path = None
ABI_VERSION = 10  # include/mm.h MM_ABI_VERSION


def load_library(path=None):
    """Load the HIP product library; raises if it is missing (no fallback).
    MM355_LIB overrides the path (A/B builds of the same library)."""
    global _lib, _lib_path
    if _lib is not None:
        return _lib
    path = path or os.environ.get("MM355_LIB") or LIB_PATH
    if not os.path.exists(path):
        raise MMError(-3, f"HIP library not built: {path} (run __graft_entry__.build())")
    L = ctypes.CDLL(path)
    vp, ci, cf, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    pp = ctypes.POINTER(Params)
    ps = ctypes.POINTER(Surface)
    sigs = {
        "mm_surface_tight": (ci, [ci, ci, ci, ps]),
        "mm_surface_aligned": (ci, [ci, ci, ci, sz, ci, ps]),
        "mm_surface_bytes": (ci, [ci, ci, ps, ctypes.POINTER(sz)]),
        "mm_process_surface": (ci, [vp, vp, ps, vp, ps, ci, vp]),
        "mm_process_stream_surfaces": (ci, [vp, vp, ps, vp, ps, ci, vp]),
        "mm_compute_state_surface": (ci, [vp, vp, ps, vp, sz, vp]),
        "mm_convert_supported": (ci, [ci, ci]),
        "mm_process_convert": (ci, [vp, vp, ps, vp, ps, ci, vp]),
        "mm_process_stream_convert": (ci, [vp, vp, ps, vp, ps, ci, vp]),
        "mm_set_lanes": (ci, [vp, ci]),
        "mm_get_lanes": (ci, [vp, ctypes.POINTER(ci)]),
        "mm_process_lanes": (ci, [vp, vp, ps, vp, ps, vp]),
        "mm_reset_lane": (ci, [vp, ci]),
        "mm_get_lane_state": (ci, [vp, ci, vp, sz, vp]),
        "mm_set_lane_state": (ci, [vp, ci, vp, sz, vp]),
        "mm_process_lanes_mask": (ci, [vp, ctypes.c_uint64, vp, ps, vp, ps, vp]),
        "mm_lanes_with_state": (ci, [vp, ctypes.POINTER(ctypes.c_uint64)]),
        "mm_set_hold": (ci, [vp, ci]),
        "mm_get_hold": (ci, [vp, ctypes.POINTER(ci)]),
        "mm_set_lanes_hold": (ci, [vp, ctypes.c_uint64]),
        "mm_get_lanes_hold": (ci, [vp, ctypes.POINTER(ctypes.c_uint64)]),
        "mm_abi_version": (ci, []),
        "mm_strerror": (ctypes.c_char_p, [ci]),
        "mm_params_default": (ci, [pp]),
        "mm_create": (ci, [ci, ci, pp, ci, ctypes.POINTER(vp)]),
        "mm_set_params": (ci, [vp, pp]),
        "mm_get_params": (ci, [vp, pp]),
        "mm_padded_size": (ci, [vp, ctypes.POINTER(ci)]),
        "mm_frame_bytes": (ci, [ci, ci, ci, ctypes.POINTER(sz)]),
        "mm_nv12_chroma_matrix": (ci, [ctypes.POINTER(ctypes.c_double)]),
        "mm_ycbcr_matrix": (ci, [ci, ctypes.POINTER(ctypes.c_double)]),
        "mm_process": (ci, [vp, vp, vp, ci, ci, vp]),
        "mm_process_stream": (ci, [vp, vp, vp, ci, ci, vp]),
        "mm_reset": (ci, [vp]),
        "mm_state_size": (ci, [vp, ctypes.POINTER(sz)]),
        "mm_get_state": (ci, [vp, vp, sz, vp]),
        "mm_set_state": (ci, [vp, vp, sz, vp]),
        "mm_compute_state": (ci, [vp, vp, ci, vp, sz, vp]),
        "mm_stream": (vp, [vp]),
        "mm_set_batch": (ci, [vp, ci]),
        "mm_get_batch": (ci, [vp, ctypes.POINTER(ci)]),
        "mm_destroy": (None, [vp]),
        "mm_synth_frames": (ci, [vp, ci, ci, ci, ci, ctypes.c_uint64, ci, vp]),
        "mm_resample_table": (ci, [ci, ci, ci, ci, ctypes.POINTER(ctypes.c_int32),
                                   ctypes.POINTER(cf)]),
        "mm_import_frames": (ci, [vp, ci, sz, sz, ctypes.POINTER(vp)]),
        "mm_ext_frames_ptr": (vp, [vp]),
        "mm_release_frames": (ci, [vp]),
        "mm_profile_begin": (ci, [vp]),
        "mm_profile_end": (ci, [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ci),
                                ctypes.POINTER(ci)]),
    }
    abi = L.mm_abi_version()
    for name, (res, args) in sigs.items():
        if abi < 5 and name in ("mm_set_batch", "mm_get_batch"):
            continue
        if abi < 6 and name in ("mm_import_frames", "mm_ext_frames_ptr", "mm_release_frames"):
            continue
        if abi < 10 and name == "mm_frame_bytes":
            continue
        if name in ("mm_nv12_chroma_matrix", "mm_ycbcr_matrix") and not hasattr(L, name):
            continue    # an A/B build from before the NV12 formats or the matrix bits (same ABI version)
        if name in SURFACE_SYMBOLS and not hasattr(L, name):
            continue    # ... or from before the pitched surfaces
        if name in CONVERT_SYMBOLS and not hasattr(L, name):
            continue    # ... or from before the format conversion
        if name in LANES_SYMBOLS and not hasattr(L, name):
            continue    # ... or from before the lanes
        if name in LANES_MASK_SYMBOLS and not hasattr(L, name):
            continue    # ... or from before the lane masks
        if name in HOLD_SYMBOLS and not hasattr(L, name):
            continue    # ... or from before the held reference
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    # mm_params grows only at its end: an older library (ABI >= 2) reads a prefix
    # of Params (A/B builds); a newer one than this binding is refused.
    if abi > ABI_VERSION or abi < 2:
        raise MMError(-1, f"{path}: ABI {abi}, binding expects <= {ABI_VERSION}")
    _lib = L
    _lib_path = os.path.realpath(path)
    return L


def library_path():
    """Real path of the libmm355 build this process loaded (MM355_LIB or the tree's)."""
    load_library()
    return _lib_path


def lib():
    return load_library()


def strerror(code):
    return lib().mm_strerror(code).decode()


def check(rc, what):
    if rc != 0:
        raise MMError(rc, what)


def abi_symbols():
    """Function names declared in include/mm.h."""
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mm_[a-z_0-9]+)\s*\(", txt)))


def frame_bytes(width, height, fmt):
    """mm_frame_bytes: bytes of one W x H frame of `fmt`."""
    n = ctypes.c_size_t()
    check(lib().mm_frame_bytes(width, height, fmt, ctypes.byref(n)), "mm_frame_bytes")
    return n.value


def nv12_chroma_matrix():
    """mm_nv12_chroma_matrix: the NV12 compose's (cb, cr) -> (I, Q) matrix,
    [[I_cb, I_cr], [Q_cb, Q_cr]] (float64)."""
    m = (ctypes.c_double * 4)()
    check(lib().mm_nv12_chroma_matrix(m), "mm_nv12_chroma_matrix")
    return np.array([[m[0], m[2]], [m[1], m[3]]])


def base_format(fmt):
    """The format without its matrix bit, and BGR24 without its byte-order bit:
    what decides a frame's size and shape.  (The plane-layout bit stays: I420
    and NV12 frames have the same size and not the same shape of planes; so
    does the low-bits bit of I010.  So does ORDER_BGRA: BGRA8 and BGRA8_SRGB have
    FORMAT_BPP entries of their own and are named with fmt=, which RGBA8 is not.)"""
    if fmt == BGR24:
        return RGB24
    return fmt & ~(MATRIX_BT709 | MATRIX_BT2020)


def ycbcr_matrix(fmt):
    """mm_ycbcr_matrix: a 4:2:0 format's (cb, cr) -> (Y, I, Q) matrix,
    [[Y_cb, Y_cr], [I_cb, I_cr], [Q_cb, Q_cr]] (float64); the Y row is what the
    decoded pixel's RGBToYIQ luma adds to y (zero for the BT.601 codes)."""
    if not hasattr(lib(), "mm_ycbcr_matrix"):
        raise MMError(-2, f"{library_path()} has no mm_ycbcr_matrix (a build from before the matrix bits)")
    m = (ctypes.c_double * 6)()
    check(lib().mm_ycbcr_matrix(fmt, m), "mm_ycbcr_matrix")
    return np.array([[m[0], m[3]], [m[1], m[4]], [m[2], m[5]]])


def resample_table(width, height, axis, edge_mode=EDGE_REPEAT):
    n = width if axis == 0 else height
    idx = np.zeros((n, 4), np.int32)
    w = np.zeros((n, 4), np.float32)
    check(lib().mm_resample_table(width, height, axis, edge_mode,
                                  idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                  w.ctypes.data_as(ctypes.POINTER(ctypes.c_float))),
          "mm_resample_table")
    return idx, w


def _ptr(x):
    """Device/host address of a torch tensor, numpy array or int."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    raise TypeError(f"cannot take the address of {type(x)}")


class Handle:
    """One mm_handle (one video stream on one GPU)."""

    def __init__(self, width, height, params=None, device=0):
        self.width, self.height = width, height
        self.params = params if params is not None else Params.make()
        h = ctypes.c_void_p()
        check(lib().mm_create(width, height, ctypes.byref(self.params), device, ctypes.byref(h)),
              "mm_create")
        self.h = h
        n = ctypes.c_int()
        check(lib().mm_padded_size(self.h, ctypes.byref(n)), "mm_padded_size")
        self.N = n.value

    @property
    def state_bytes(self):
        """mm_state_size: follows the current parameters (the steerable mode's
        state depends on levels, orientations and temporal filter)."""
        s = ctypes.c_size_t()
        check(lib().mm_state_size(self.h, ctypes.byref(s)), "mm_state_size")
        return s.value

    def set_batch(self, frames):
        check(lib().mm_set_batch(self.h, int(frames)), "mm_set_batch")

    @property
    def batch(self):
        n = ctypes.c_int()
        check(lib().mm_get_batch(self.h, ctypes.byref(n)), "mm_get_batch")
        return n.value

    def close(self):
        if getattr(self, "h", None):
            lib().mm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self):
        return lib().mm_stream(self.h)

    def set_params(self, params):
        self.params = params
        check(lib().mm_set_params(self.h, ctypes.byref(params)), "mm_set_params")

    def process(self, src, dst, fmt, on_device=True, stream=None):
        check(lib().mm_process(self.h, _ptr(src), _ptr(dst), fmt,
                               FRAMES_ON_DEVICE if on_device else 0, _ptr(stream)),
              "mm_process")

    def process_stream(self, src, dst, count, fmt, stream=None):
        check(lib().mm_process_stream(self.h, _ptr(src), _ptr(dst), count, fmt, _ptr(stream)),
              "mm_process_stream")

    def process_surface(self, src, src_layout, dst, dst_layout, on_device=True, stream=None):
        """mm_process_surface: one frame, each side in its own Surface."""
        check(_surface_fn("mm_process_surface")(self.h, _ptr(src), ctypes.byref(src_layout), _ptr(dst),
                                                ctypes.byref(dst_layout),
                                                FRAMES_ON_DEVICE if on_device else 0, _ptr(stream)),
              "mm_process_surface")

    def process_stream_surfaces(self, src, src_layout, dst, dst_layout, count, stream=None):
        """mm_process_stream_surfaces: frame k at k * frame_stride of its side."""
        check(_surface_fn("mm_process_stream_surfaces")(self.h, _ptr(src), ctypes.byref(src_layout),
                                                        _ptr(dst), ctypes.byref(dst_layout), count,
                                                        _ptr(stream)), "mm_process_stream_surfaces")

    def process_convert(self, src, src_layout, dst, dst_layout, on_device=True, stream=None):
        """mm_process_convert: one frame in src_layout.format, out in
        dst_layout.format (convert_supported)."""
        check(_convert_fn("mm_process_convert")(self.h, _ptr(src), ctypes.byref(src_layout), _ptr(dst),
                                                ctypes.byref(dst_layout),
                                                FRAMES_ON_DEVICE if on_device else 0, _ptr(stream)),
              "mm_process_convert")

    def process_stream_convert(self, src, src_layout, dst, dst_layout, count, stream=None):
        """mm_process_stream_convert: frame k at k * frame_stride of its side."""
        check(_convert_fn("mm_process_stream_convert")(self.h, _ptr(src), ctypes.byref(src_layout),
                                                       _ptr(dst), ctypes.byref(dst_layout), count,
                                                       _ptr(stream)), "mm_process_stream_convert")

    def set_lanes(self, n):
        """mm_set_lanes: n live streams' states on this handle (0 frees them)."""
        check(_lanes_fn("mm_set_lanes")(self.h, int(n)), "mm_set_lanes")

    def lanes(self):
        n = ctypes.c_int()
        check(_lanes_fn("mm_get_lanes")(self.h, ctypes.byref(n)), "mm_get_lanes")
        return n.value

    def process_lanes(self, src, src_layout, dst, dst_layout, stream=None):
        """mm_process_lanes: one frame of every lane; lane k's frame at
        k * frame_stride of its side."""
        check(_lanes_fn("mm_process_lanes")(self.h, _ptr(src), ctypes.byref(src_layout), _ptr(dst),
                                            ctypes.byref(dst_layout), _ptr(stream)), "mm_process_lanes")

    def process_lanes_mask(self, mask, src, src_layout, dst, dst_layout, stream=None):
        """mm_process_lanes_mask: one frame of each lane whose bit of `mask` is
        set; lane k's frame at k * frame_stride of its side, whatever the mask."""
        check(_lanes_mask_fn("mm_process_lanes_mask")(self.h, int(mask), _ptr(src), ctypes.byref(src_layout),
                                                      _ptr(dst), ctypes.byref(dst_layout), _ptr(stream)),
              "mm_process_lanes_mask")

    def lanes_with_state(self):
        """mm_lanes_with_state: bit k set where lane k has state."""
        m = ctypes.c_uint64()
        check(_lanes_mask_fn("mm_lanes_with_state")(self.h, ctypes.byref(m)), "mm_lanes_with_state")
        return m.value

    def reset_lane(self, lane=-1):
        """mm_reset_lane: lane's next frame passes through (-1: every lane's)."""
        check(_lanes_fn("mm_reset_lane")(self.h, int(lane)), "mm_reset_lane")

    def get_lane_state(self, lane, dev_buf, stream=None):
        check(_lanes_fn("mm_get_lane_state")(self.h, int(lane), _ptr(dev_buf), self.state_bytes,
                                             _ptr(stream)), "mm_get_lane_state")

    def set_lane_state(self, lane, dev_buf, stream=None):
        check(_lanes_fn("mm_set_lane_state")(self.h, int(lane), _ptr(dev_buf), self.state_bytes,
                                             _ptr(stream)), "mm_set_lane_state")

    def set_hold(self, on):
        """mm_set_hold: from the next call, frames pair with the state the
        handle has and do not advance it (a held reference frame)."""
        check(_hold_fn("mm_set_hold")(self.h, int(on)), "mm_set_hold")

    def hold(self):
        v = ctypes.c_int()
        check(_hold_fn("mm_get_hold")(self.h, ctypes.byref(v)), "mm_get_hold")
        return bool(v.value)

    def set_lanes_hold(self, mask):
        """mm_set_lanes_hold: bit k set makes lane k hold its reference."""
        check(_hold_fn("mm_set_lanes_hold")(self.h, int(mask)), "mm_set_lanes_hold")

    def lanes_hold(self):
        m = ctypes.c_uint64()
        check(_hold_fn("mm_get_lanes_hold")(self.h, ctypes.byref(m)), "mm_get_lanes_hold")
        return m.value

    def reset(self):
        check(lib().mm_reset(self.h), "mm_reset")

    def get_state(self, dev_buf, stream=None):
        check(lib().mm_get_state(self.h, _ptr(dev_buf), self.state_bytes, _ptr(stream)),
              "mm_get_state")

    def set_state(self, dev_buf, stream=None):
        check(lib().mm_set_state(self.h, _ptr(dev_buf), self.state_bytes, _ptr(stream)),
              "mm_set_state")

    def compute_state(self, src, fmt, dev_buf, stream=None):
        check(lib().mm_compute_state(self.h, _ptr(src), fmt, _ptr(dev_buf), self.state_bytes,
                                     _ptr(stream)), "mm_compute_state")

    def compute_state_surface(self, src, src_layout, dev_buf, stream=None):
        check(_surface_fn("mm_compute_state_surface")(self.h, _ptr(src), ctypes.byref(src_layout),
                                                      _ptr(dev_buf), self.state_bytes, _ptr(stream)),
              "mm_compute_state_surface")

    def profile_begin(self):
        check(lib().mm_profile_begin(self.h), "mm_profile_begin")

    def profile_end(self):
        """-> {kernel: (total_ms, launches, frames)} for every kernel of the path."""
        k = len(KERNELS)
        ms = (ctypes.c_double * k)()
        n = (ctypes.c_int * k)()
        f = (ctypes.c_int * k)()
        check(lib().mm_profile_end(self.h, ms, n, f), "mm_profile_end")
        return {name: (ms[k], n[k], f[k]) for k, name in enumerate(KERNELS)}

    def synth(self, dev_out, t0, count, seed=0x5EED0000, gray=False, stream=None):
        check(lib().mm_synth_frames(_ptr(dev_out), self.width, self.height, t0, count, seed,
                                    1 if gray else 0, _ptr(stream)), "mm_synth_frames")
