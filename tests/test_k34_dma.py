"""k_rows_inv_compose with its source rows staged in LDS (csrc/mm_kernels.hpp,
SRCDMA): the RGBA8 formats' compose reads the four new source rows of a strip
step from rows that an LDS-DMA copied under the step's inverse FFT, where every
source row of the launch is 16-byte aligned (csrc/mm_impl.hpp k34_src_dma);
other layouts keep the register loads.

The staged pixels are the pixels the loads returned and the expressions are
unchanged, so the fused kernel must still equal the unfused K3 -> K4 pair
(MM_K34_ROWS=0) bit for bit.  Streams of 3 frames: the launch starts at frame
1.  Shapes: one-wave workgroups with a partial last strip, clamped rows and
neighbour pixels that wrap to the far end of a row (200 x 120); the tightest
canvas margin (504 at N = 512); clamped quads in the last wave (1016 = N - 8 at
N = 1024); multi-wave FFT groups, where a neighbour pixel is another wave's
copy (1032 at N = 2048); the N = 4096 instance with its staged rows past 64 KB
of LDS (2056).
"""
import functools

import numpy as np
import pytest

import mmtest as T
import surface as SF

pytestmark = pytest.mark.gpu


def _run(rows, W, H, fr, levels=5, edge=0, **kw):
    with SF.env(MM_K34_ROWS=str(rows)):
        return T.gpu_run(W, H, fr, levels, 25.0, edge, mode="stream", **kw)


@functools.lru_cache(maxsize=None)
def _frames(W, H):
    fr = T.synth(W, H, 3, fmt="u8")
    for f in fr:
        f.setflags(write=False)
    return tuple(fr)


@functools.lru_cache(maxsize=None)
def _unfused(W, H, edge, srgb=False):
    import mm355
    got = _run(0, W, H, list(_frames(W, H)), edge=edge, fmt=mm355.RGBA8_SRGB if srgb else None)
    for g in got:
        g.setflags(write=False)
    return tuple(got)


def _same(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), (k, int((x != y).sum()))


@pytest.mark.parametrize("W,H,rows,edge", [
    (200, 120, 16, 0), (200, 120, 16, 1), (200, 120, 64, 0), (200, 120, 64, 1),
    (504, 40, 16, 0), (1016, 72, 16, 1), (1032, 48, 16, 0), (2056, 32, 16, 1)])
def test_staged_rows_equal_unfused_bitwise(W, H, rows, edge):
    got = _run(rows, W, H, list(_frames(W, H)), edge=edge)
    assert np.array_equal(got[0], _frames(W, H)[0])
    _same(got, _unfused(W, H, edge))


def test_srgb8_equals_unfused_bitwise():
    import mm355
    W, H = 200, 120
    got = _run(16, W, H, list(_frames(W, H)), fmt=mm355.RGBA8_SRGB)
    _same(got, _unfused(W, H, 0, srgb=True))


def test_standard_mode_equals_unfused_bitwise():
    W, H = 200, 120
    fr, std = list(_frames(W, H)), {"apply": True}
    _same(_run(16, W, H, fr, standard=std), _run(0, W, H, fr, standard=std))


def test_unaligned_surface_equals_packed_bitwise():
    """An input surface 4 mod 16 from an aligned base with a pitch of row
    bytes + 4 (804): its quads are not 16-byte aligned, so the launch keeps
    the register loads; the packed stream takes the staged rows.  Same
    results."""
    W, H, name = 200, 120, "rgba8"
    fr = SF.tight_frames(name, W, H, 3)
    lin = SF.lay_plus_unit(name, W, H)
    assert lin.pitch % 16 == 4
    with SF.env(MM_K34_ROWS="16"):
        got = SF.run_pitched(name, W, H, fr, lin, SF.lay_tight(name, W, H), mode="stream", in_base=4)
        want = SF.run_tight(name, W, H, fr, mode="stream")
    SF.assert_same(got, want, "unaligned input surface")


def test_staged_rows_vs_oracle():
    W, H = 240, 136
    fr = list(_frames(W, H))
    ref = T.oracle_run(W, H, fr, 5, 25.0, 1)
    got = _run(64, W, H, fr, edge=1)
    assert np.array_equal(got[0], fr[0])
    for g, r in zip(got[1:], ref[1:]):
        T.assert_close_u8(g, r)
