"""mm355 — Python host mirror of the MI355X-native MotionMagnificationProcessor.

The product is the C-ABI library ``lib/libmm355.so`` (include/mm.h) whose HIP
kernels do all the work.  This module binds it with ctypes and mirrors the
reference Unity component's operator surface
(Assets/Scripts/MotionMagnificationProcessor.cs) so a user of the reference
finds the same names, argument meaning and error behaviour:

    proc = MotionMagnificationProcessor(width, height, pyramid_levels=5,
                                        phase_scale=25.0)
    proc.Start()                       # .cs:90  -> mm_create
    proc.OnRenderImage(src, dst)       # .cs:101 -> mm_process
    proc.phase_scale = 10.0; proc.OnValidate()   # .cs:78 -> mm_set_params
    proc.OnDestroy()                   # .cs:96  -> mm_destroy

There is no CPU fallback.  If the library or a gfx950 device is missing,
construction/Start raises ``MMError`` — loudly, never silently.
"""
from .binding import (MMError, lib, load_library, LIB_PATH, RGBA8, RGBA32F, RGBA16F, RGBA8_SRGB,
                      NV12, NV12_FULL, P010, P010_FULL, MATRIX_BT709, MATRIX_BT2020, FORMAT_BPP, frame_bytes,
                      Y8, Y10, Y12, Y16, MONO_FORMATS, MONO_BITS,
                      RGB24, BGR24, ORDER_BGR, RGB24_FORMATS, BGRA8, BGRA8_SRGB, ORDER_BGRA, BGRA_FORMATS, has_bgra,
                      I420, I420_FULL, PLANAR, I420_FORMATS,
                      I010, I010_FULL, LOW_BITS, I010_FORMATS,
                      YUY2, YUY2_FULL, UYVY, UYVY_FULL, PACKED422_FORMATS,
                      Y210, Y210_FULL, Y210_FORMATS,
                      V210, V210_FULL, PACK_V210, V210_FORMATS, FORMAT_GROUP, row_bytes, tight_pitch,
                      nv12_chroma_matrix, ycbcr_matrix, base_format,
                      EDGE_REPEAT, EDGE_CLAMP, MODE_PYRAMID, MODE_STANDARD, MODE_STEERABLE,
                      FILTER_DIFF, FILTER_IIR, Params, Handle, Surface, has_surfaces,
                      convert_supported, has_convert, has_lanes, has_lanes_mask, has_hold, LANES_MAX, abi_symbols, resample_table,
                      strerror)
from .processor import MotionMagnificationProcessor, frame_layout
from .stream import ShardedStream, shard_range
from .ring import Ring, new_ring_id, ring_lib

__all__ = ["MMError", "lib", "load_library", "LIB_PATH", "RGBA8", "RGBA32F", "RGBA16F",
           "RGBA8_SRGB", "NV12", "NV12_FULL", "P010", "P010_FULL", "FORMAT_BPP", "frame_bytes",
           "Y8", "Y10", "Y12", "Y16", "MONO_FORMATS", "MONO_BITS",
           "RGB24", "BGR24", "ORDER_BGR", "RGB24_FORMATS", "BGRA8", "BGRA8_SRGB", "ORDER_BGRA", "BGRA_FORMATS", "has_bgra",
           "I420", "I420_FULL", "PLANAR", "I420_FORMATS",
           "I010", "I010_FULL", "LOW_BITS", "I010_FORMATS",
           "YUY2", "YUY2_FULL", "UYVY", "UYVY_FULL", "PACKED422_FORMATS",
           "Y210", "Y210_FULL", "Y210_FORMATS",
           "V210", "V210_FULL", "PACK_V210", "V210_FORMATS", "FORMAT_GROUP", "row_bytes", "tight_pitch",
           "MATRIX_BT709", "MATRIX_BT2020", "nv12_chroma_matrix", "ycbcr_matrix", "base_format",
           "EDGE_REPEAT", "EDGE_CLAMP", "MODE_PYRAMID", "MODE_STANDARD", "MODE_STEERABLE",
           "FILTER_DIFF", "FILTER_IIR", "Params", "Handle", "Surface", "has_surfaces",
           "convert_supported", "has_convert", "has_lanes", "has_lanes_mask", "has_hold", "LANES_MAX",
           "frame_layout", "abi_symbols",
           "resample_table", "strerror", "MotionMagnificationProcessor",
           "ShardedStream", "shard_range", "Ring", "new_ring_id", "ring_lib"]
