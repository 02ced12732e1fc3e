"""Mirror of the reference Unity component ``MotionMagnificationProcessor``
(Assets/Scripts/MotionMagnificationProcessor.cs) on top of the C-ABI.

Field names follow the reference's serialized inspector fields (.cs:7-43) in
snake_case; methods keep the reference's Unity callback names.
"""
import numpy as np

from .binding import (EDGE_REPEAT, FILTER_DIFF, MODE_PYRAMID, MODE_STANDARD, MODE_STEERABLE,
                      MONO_FORMATS, NV12, NV12_FULL, P010, P010_FULL, PACKED422_FORMATS, RGBA8, RGBA8_SRGB, RGBA16F,
                      BGRA_FORMATS, I010_FORMATS, I420_FORMATS, RGB24_FORMATS, RGBA32F, V210, V210_FORMATS, Y8, Y210_FORMATS,
                      Handle, MMError, Params, Surface, base_format, convert_supported, has_hold, tight_pitch)


def _fmt_of(frame, srgb=False):
    """Frame format from the dtype: uint8 UNORM (or sRGB-encoded with srgb),
    float16 (linear half, the HDR camera target), float32.  (A bare uint8 frame
    is RGBA8: the grayscale formats are always named, OnRenderImage's fmt=.
    An [H, W, 3] frame must be named too: its byte order cannot be guessed.)"""
    dt = str(getattr(frame, "dtype", ""))
    shape = tuple(getattr(frame, "shape", ()))
    if len(shape) == 3 and shape[2] == 3:
        raise MMError(-1, f"frame shape {shape}: a three-channel frame needs fmt=mm355.RGB24 "
                          "(bytes R G B) or fmt=mm355.BGR24 (B G R, OpenCV's order)")
    if dt.endswith("uint8"):
        return RGBA8_SRGB if srgb else RGBA8
    if dt.endswith("float16"):
        return RGBA16F
    if dt.endswith("float32"):
        return RGBA32F
    raise MMError(-1, f"frame dtype {dt} (want uint8, float16 or float32 RGBA)")


def _is_device(frame):
    return bool(getattr(frame, "is_cuda", False))


# One row per family of formats: what a frame of it looks like as an array.
#   shape(H, W); dtype name (None: the frame's own, any RGBA dtype); the inner
#   strides in items, innermost last; whether rows may lie a pitch apart (else
#   the frame is contiguous: its planes have no room for one); the error's wording
_CONTIGUOUS_3P = "a three-plane 4:2:0 frame must be contiguous (name a Surface through Handle.process_surface)"
_FAMILIES = {
    "rgba": (lambda h, w: (h, w, 4), None, (4, 1), True, "pixels and channels packed"),
    "rgb24": (lambda h, w: (h, w, 3), "uint8", (3, 1), True, "pixels and channels packed"),   # rows at any byte
    "bgra": (lambda h, w: (h, w, 4), "uint8", (4, 1), True, "pixels and channels packed"),    # RGBA8's rows, bytes B G R A
    "y8": (lambda h, w: (h, w), "uint8", (1,), True, "samples packed"),
    "y16": (lambda h, w: (h, w), "uint16", (1,), True, "samples packed"),
    # [H, 2 W]: rows of W / 2 macropixels, four bytes or (Y210) four words Y0 Cb Y1 Cr
    "yuv422": (lambda h, w: (h, 2 * w), "uint8", (1,), True, "bytes packed"),
    "y210": (lambda h, w: (h, 2 * w), "uint16", (1,), True, "words packed"),
    # [H, pitch / 4] dwords of three 10-bit codes, pitch = 128 * ceil(W / 48): the
    # frame as capture SDKs and ffmpeg lay it out, row padding included
    "v210": (lambda h, w: (h, tight_pitch(w, V210) // 4), "uint32", (1,), True, "dwords packed"),
    # one contiguous [H * 3 / 2, W] array: H luma rows, then H / 2 rows of chroma
    # (one (Cb, Cr) plane, or a Cb and a Cr plane), in bytes or 16-bit words
    # (the two-plane rows: shape and dtype only, for _convert_side and host_frames.  Such
    # a frame is never named to frame_layout, which holds it to the RGBA row.)
    "nv12": (lambda h, w: (h * 3 // 2, w), "uint8", None, None, None),
    "p010": (lambda h, w: (h * 3 // 2, w), "uint16", None, None, None),
    "i420": (lambda h, w: (h * 3 // 2, w), "uint8", (1,), False, _CONTIGUOUS_3P),
    "i010": (lambda h, w: (h * 3 // 2, w), "uint16", (1,), False, _CONTIGUOUS_3P),
}


def _family(fmt):
    if fmt in RGB24_FORMATS:
        return "rgb24"
    if fmt in BGRA_FORMATS:
        return "bgra"
    if fmt in MONO_FORMATS:
        return "y8" if fmt == Y8 else "y16"
    base = base_format(fmt)         # a matrix bit changes no size or shape
    for name, codes in (("yuv422", PACKED422_FORMATS), ("y210", Y210_FORMATS), ("v210", V210_FORMATS),
                        ("i420", I420_FORMATS),
                        ("i010", I010_FORMATS), ("nv12", (NV12, NV12_FULL)), ("p010", (P010, P010_FULL))):
        if base in codes:
            return name
    return "rgba"


def frame_layout(frame, width, height, fmt):
    """The mm_surface of a row-strided frame (torch tensor or numpy array) in
    its format's shape (RGBA: [H, W, 4]): channels and pixels packed, rows any
    valid pitch apart, so that a region of interest is ``parent[y:y+H, x:x+W]``.
    None for a contiguous frame (the tight entry point); MMError for any other
    striding.  Needs no GPU.  (A two-plane 4:2:0 frame is no frame of this call:
    it is held to the RGBA shape.)"""
    fam = _family(fmt)
    shape, dtype, inner, pitched, packed = _FAMILIES["rgba" if fam in ("nv12", "p010") else fam]
    if isinstance(frame, np.ndarray):
        item = frame.itemsize
        strides = tuple(frame.strides)                       # bytes
    else:
        item = frame.element_size()
        strides = tuple(s * item for s in frame.stride())    # elements -> bytes
    want = shape(height, width)
    if dtype is None:
        if tuple(frame.shape) != want:
            raise MMError(-1, f"frame shape {tuple(frame.shape)} (want {want})")
    elif tuple(frame.shape) != want or not str(frame.dtype).endswith(dtype):
        raise MMError(-1, f"frame {tuple(frame.shape)} {frame.dtype} (want {want} {dtype})")
    row = item * int(np.prod(want[1:]))
    if not pitched:
        if strides != (row, item):
            raise MMError(-1, packed)
        return None
    if strides[1:] != tuple(i * item for i in inner) or strides[0] <= 0:
        raise MMError(-1, f"frames must be contiguous or row-strided ({packed})")
    if strides[0] == row:
        return None
    lay = Surface(format=fmt, pitch=strides[0], chroma_offset=0, chroma_pitch=0, frame_stride=0)
    lay.bytes(width, height)    # mm_surface_bytes: the pitch's validation (a multiple of the format's unit)
    return lay


def _convert_side(frame, width, height, fmt, side):
    """One side of a convert call, checked by that side's format: a 4:2:0 frame
    is one contiguous [H * 3 / 2, W] array, uint8 (NV12 codes) or uint16 (P010
    codes: the words as they lie); an RGBA8 frame is [H, W, 4] uint8, contiguous
    or row-strided.  -> its Surface.  MMError on any mismatch, before any frame
    call into the library."""
    fam = _family(fmt)
    shape, dtype = _FAMILIES[fam][0](height, width), _FAMILIES[fam][1] or "uint8"
    if tuple(frame.shape) != shape or not str(frame.dtype).endswith(dtype):
        raise MMError(-1, f"{side} {tuple(frame.shape)} {frame.dtype} (want {shape} {dtype} for format {fmt})")
    if fam in ("nv12", "p010"):
        contiguous = frame.flags["C_CONTIGUOUS"] if isinstance(frame, np.ndarray) else frame.is_contiguous()
        if not contiguous:
            raise MMError(-1, f"{side}: a 4:2:0 frame must be contiguous (name a Surface through Handle.process_convert)")
        return Surface.tight(width, height, fmt)
    return frame_layout(frame, width, height, fmt) or Surface.tight(width, height, fmt)


class MotionMagnificationProcessor:
    """[RequireComponent(typeof(Camera))] class MotionMagnificationProcessor (.cs:4-5).

    ``width``/``height`` play the role of Screen.width/height read in
    InitializeProcessor (.cs:298-299): geometry is frozen at Start().
    """

    def __init__(self, width, height, *, apply_motion_magnification=True,
                 show_magnitude=False, show_phase=False, use_pyramid_decomposition=True,
                 pyramid_levels=5, min_frequency=0.05, max_frequency=0.45,
                 phase_scale=10.0, magnitude_threshold=0.01, apply_bandpass_filter=True,
                 low_frequency_cutoff=0.05, high_frequency_cutoff=0.4, filter_steepness=3.0,
                 motion_sensitivity=1.5, enhance_edges=True, edge_enhancement=0.8,
                 edge_mode=EDGE_REPEAT, orientations=1, temporal_filter=FILTER_DIFF,
                 iir_low=None, iir_high=None, srgb=False, hold_reference=False, device=0):
        self.width, self.height, self.device = width, height, device
        # 8-bit frames are sRGB-encoded render targets under Unity's Linear colour
        # space (ProjectSettings/ProjectSettings.asset:50): decoded to linear light
        # on read and encoded on write (MM_RGBA8_SRGB); False: UNORM bytes
        self.srgb = srgb
        self.apply_motion_magnification = apply_motion_magnification  # .cs:12
        self.show_magnitude = show_magnitude                          # .cs:13
        self.show_phase = show_phase                                  # .cs:14
        self.use_pyramid_decomposition = use_pyramid_decomposition    # .cs:18
        self.pyramid_levels = pyramid_levels                          # .cs:19
        self.min_frequency = min_frequency                            # .cs:20
        self.max_frequency = max_frequency                            # .cs:21
        self.phase_scale = phase_scale                                # .cs:29
        self.magnitude_threshold = magnitude_threshold                # .cs:30
        self.apply_bandpass_filter = apply_bandpass_filter            # .cs:35
        self.low_frequency_cutoff = low_frequency_cutoff              # .cs:36
        self.high_frequency_cutoff = high_frequency_cutoff            # .cs:37
        self.filter_steepness = filter_steepness                      # .cs:38
        self.motion_sensitivity = motion_sensitivity                  # .cs:41
        self.enhance_edges = enhance_edges                            # .cs:42
        self.edge_enhancement = edge_enhancement                      # .cs:43
        self.edge_mode = edge_mode
        # steerable extension (no reference counterpart):
        # orientations 4/6/8 with the pyramid switch on select MM_MODE_STEERABLE;
        # iir_low/iir_high None keep mm_params_default's coefficients
        self.orientations = orientations
        self.temporal_filter = temporal_filter
        self.iir_low, self.iir_high = iir_low, iir_high
        # held reference frame (no reference counterpart, include/mm.h "Held
        # reference frame"): every frame pairs with one reference frame, the
        # first after Start() / reset() or the one rehold() names, instead of
        # with the frame before it; applied in Start() / OnValidate()
        self.hold_reference = hold_reference
        self._rehold = False
        self._handle = None

    # -- reference lifecycle -------------------------------------------------
    def _params(self):
        # usePyramidDecomposition selects ProcessFrameWithPyramidDecomposition or
        # ProcessFrameWithStandardMagnification (.cs:128-135)
        mode = MODE_PYRAMID if self.use_pyramid_decomposition else MODE_STANDARD
        steer = {}
        if self.use_pyramid_decomposition and self.orientations != 1:
            mode = MODE_STEERABLE
            steer = dict(orientations=self.orientations, temporal_filter=self.temporal_filter)
            if self.iir_low is not None:
                steer["iir_low"] = self.iir_low
            if self.iir_high is not None:
                steer["iir_high"] = self.iir_high
        return Params.make(levels=self.pyramid_levels, min_freq=self.min_frequency,
                           max_freq=self.max_frequency, phase_scale=self.phase_scale,
                           magnitude_threshold=self.magnitude_threshold,
                           edge_mode=self.edge_mode,
                           apply_magnification=self.apply_motion_magnification, mode=mode,
                           apply_bandpass_filter=self.apply_bandpass_filter,
                           low_frequency_cutoff=self.low_frequency_cutoff,
                           high_frequency_cutoff=self.high_frequency_cutoff,
                           filter_steepness=self.filter_steepness,
                           motion_sensitivity=self.motion_sensitivity,
                           enhance_edges=self.enhance_edges,
                           edge_enhancement=self.edge_enhancement,
                           # showMagnitude / showPhase: ProcessDebugView (.cs:119-123)
                           show_magnitude=self.show_magnitude, show_phase=self.show_phase,
                           **steer)

    def Start(self):
        """Start -> InitializeProcessor (.cs:90-94, :289-342). Raises on failure."""
        self._handle = Handle(self.width, self.height, self._params(), self.device)
        if self.hold_reference:
            self._handle.set_hold(True)
        return self

    def OnValidate(self):
        """OnValidate (.cs:78-88): push edited fields; effective next frame."""
        if self._handle is not None:
            self._handle.set_params(self._params())
            # (a library from before the hold has nothing to switch off)
            if self.hold_reference or has_hold():
                self._handle.set_hold(self.hold_reference)

    def OnRenderImage(self, source, destination, fmt=None, dst_fmt=None):
        """OnRenderImage (.cs:101-143). source/destination: [H, W, 4] uint8,
        float16 or float32, both torch CUDA tensors (async on torch's current
        stream) or both host numpy arrays (synchronous).  fmt=Y8 / Y10 / Y12 /
        Y16: grayscale camera frames, [H, W] uint8 (Y8) or uint16 on both sides
        (contiguous or row-strided views).  fmt=YUY2 / YUY2_FULL / UYVY /
        UYVY_FULL, with or without a matrix bit: packed 4:2:2 capture frames,
        [H, 2 W] uint8 on both sides (contiguous or row-strided views).
        fmt=Y210 / Y210_FULL, with or without a matrix bit: 10-bit packed 4:2:2,
        [H, 2 W] uint16 on both sides (P010's convention: the words as they lie;
        contiguous or row-strided views).  fmt=V210 / V210_FULL, with or without a
        matrix bit: v210 capture frames, [H, pitch / 4] uint32 on both sides with
        pitch = mm355.tight_pitch(W, fmt) = 128 * ceil(W / 48), the layout of
        capture SDKs and ffmpeg (contiguous, or row-strided views whose pitch is a
        multiple of 16); any other shape raises.  fmt=RGB24 / BGR24: [H, W, 3] uint8
        on both sides, as cv2 (BGR24), PIL and imageio (RGB24) hand them out:
        device tensors, contiguous or row-strided views that start at any
        byte, or host numpy arrays; such a frame without fmt= raises.
        fmt=BGRA8 / BGRA8_SRGB: [H, W, 4] uint8 on both sides, bytes B G R A as
        swap chains, desktop duplication, CoreVideo, NDI and OpenCV's four-channel
        mats hand them out: device tensors, contiguous or row-strided views, or
        host numpy arrays, as for RGBA8 (a bare uint8 frame is RGBA8: name BGRA).
        fmt=I420 / I420_FULL, with or without a matrix bit: three-plane 4:2:0,
        one contiguous [H * 3 / 2, W] uint8 array on both sides (the frame's
        bytes in NV12's shape: H luma rows, then the Cb plane, then the Cr plane).
        fmt=I010 / I010_FULL, with or without a matrix bit: its 10-bit form,
        one contiguous [H * 3 / 2, W] uint16 array on both sides (the words as
        they lie, the code in the low 10 bits).
        dst_fmt (None, or equal to fmt: the above): the destination's format
        where it differs from the source's (mm355.convert_supported): fmt=NV12 /
        P010 codes with dst_fmt=RGBA8, the source one contiguous [H * 3 / 2, W]
        uint8 / uint16 array and the destination [H, W, 4] uint8; or an [H, W, 4]
        uint8 source (fmt None or RGBA8) with dst_fmt an NV12 code; BGRA8 stands
        wherever RGBA8 does (dst_fmt=BGRA8, or fmt=BGRA8 with an NV12 dst_fmt).  Each side's
        shape and dtype are checked by that side's format, before any frame
        call into the library."""
        if self._rehold and self._handle is not None:
            # rehold(): this frame runs with hold off (it still pairs with the
            # old reference) and leaves its own state behind as the new one
            # (a frame that is refused does not use the re-reference up)
            self._rehold = False
            self._handle.set_hold(False)
            try:
                return self.OnRenderImage(source, destination, fmt, dst_fmt)
            except Exception:
                self._rehold = True
                raise
            finally:
                self._handle.set_hold(self.hold_reference)
        if dst_fmt is not None and dst_fmt != (fmt if fmt is not None else _fmt_of(source, self.srgb)):
            if fmt is None:
                fmt = _fmt_of(source, self.srgb)
            if self._handle is None:
                raise MMError(-1, "dst_fmt: no Blit between two formats before Start()")
            rc = convert_supported(fmt, dst_fmt)
            if rc:
                raise MMError(rc, f"fmt={fmt}, dst_fmt={dst_fmt}")
            on_dev = _is_device(source)
            if on_dev != _is_device(destination):
                raise MMError(-1, "source and destination must both be device or host")
            src_lay = _convert_side(source, self.width, self.height, fmt, "source")
            dst_lay = _convert_side(destination, self.width, self.height, dst_fmt, "destination")
            stream = None
            if on_dev:
                import torch
                stream = torch.cuda.current_stream(source.device).cuda_stream
            self._handle.process_convert(source, src_lay, destination, dst_lay, on_device=on_dev, stream=stream)
            return
        if self._handle is None:                       # !isInitialized -> Blit (.cs:103-107)
            destination[...] = source
            return
        if fmt is None:
            fmt = _fmt_of(source, self.srgb)
            if _fmt_of(destination, self.srgb) != fmt:
                raise MMError(-1, "source/destination formats differ")
        elif (fmt not in MONO_FORMATS and base_format(fmt) not in PACKED422_FORMATS and
              base_format(fmt) not in Y210_FORMATS and base_format(fmt) not in V210_FORMATS and
              fmt not in RGB24_FORMATS and fmt not in BGRA_FORMATS and
              base_format(fmt) not in I420_FORMATS and base_format(fmt) not in I010_FORMATS):
            raise MMError(-1, f"fmt={fmt}: only the grayscale, packed 4:2:2, packed RGB, BGRA and three-plane 4:2:0 formats are named, "
                              "the others follow the dtype")
        on_dev = _is_device(source)
        if on_dev != _is_device(destination):
            raise MMError(-1, "source and destination must both be device or host")
        # contiguous frames, or row-strided views (a region of interest of a
        # larger frame): the layout follows the strides, each side its own
        src_lay = frame_layout(source, self.width, self.height, fmt)
        dst_lay = frame_layout(destination, self.width, self.height, fmt)
        stream = None
        if on_dev:   # order after whatever produced `source` on torch's current stream
            import torch
            stream = torch.cuda.current_stream(source.device).cuda_stream
        if src_lay is None and dst_lay is None:
            self._handle.process(source, destination, fmt, on_device=on_dev, stream=stream)
            return
        tight = Surface.tight(self.width, self.height, fmt)
        self._handle.process_surface(source, src_lay or tight, destination, dst_lay or tight,
                                     on_device=on_dev, stream=stream)

    def OnDestroy(self):
        """OnDestroy -> ReleaseResources (.cs:96-99, :344-356)."""
        if self._handle is not None:
            self._handle.close()
            self._handle = None

    # -- extras ---------------------------------------------------------------
    def reset(self):
        """isFirstFrame = true (.cs:75): next frame passes through."""
        self._handle.reset()

    def rehold(self):
        """With hold_reference: the next frame becomes the new reference (one
        frame with hold off: no passthrough frame)."""
        self._rehold = True

    @property
    def handle(self):
        return self._handle

    @property
    def padded_size(self):
        return self._handle.N if self._handle else None


def host_frames(n, h, w, fmt):
    """n zeroed host frames of a format, in its family's shape and dtype"""
    shape, dtype = _FAMILIES[_family(fmt)][:2]
    dtype = dtype or {RGBA8: "uint8", RGBA8_SRGB: "uint8", RGBA16F: "float16"}.get(fmt, "float32")
    return np.zeros((n,) + shape(h, w), dtype)
