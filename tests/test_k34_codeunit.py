"""The RGBA8 compose in code units (csrc/mm_kernels.hpp yiq_rgba8): where the
output format is RGBA8 UNORM, the compose kernels blur Y' with 255-scaled
weights, run YIQToRGB with a 255-scaled matrix and leave the saturate and the
rounding to the packed byte convert (clamp to 0 .. 255, round to nearest even).

One definition serves k_compose, k_rows_inv_compose (source rows staged in LDS
or loaded to registers) and k_rows_inv_compose4, so the three forms must agree
bit for bit, and each must stay within the RGBA8 bar against the C oracle
(tests/mmtest.py assert_close_u8: at most 1 code, on at most
0.1 % of a frame's values), which truncates r * 255 + 0.5 of the saturated
value instead.

Shapes, the smallest that reach each instance of the fused kernel (even sizes,
W % 8 == 0, N - W >= 8, N - H >= 4), 5 frames, both edge modes, the stream call
and frame calls:
  136 x 20   N = 256: FFT groups of half a wave
  520 x 24   N = 1024
  1040 x 16, 1928 x 12   N = 2048: the benchmark's instance, source rows staged
  1040 x 16 through an input surface whose pitch (4164) is no multiple of 16:
             the same instance with register loads
Strips of 8 rows: several strips, a partial last one.

Content: the synthetic frames, and one stream of saturating content (every
channel 0 or 255 in blocks that move) so that both ends of the clamp, and the
alpha byte beside a clamped blue, are exercised.

The cap is the bar itself, not what the kernels give.  Measured on the CPU on
exactly these inputs, the C oracle against its float64 twin
(tests/np_twin.py process_frame, encoded as floor(v * 255 + 0.5)): see
TWIN_VS_ORACLE below, worst frame of each stream.  No assembly is inspected.
"""
import functools

import numpy as np
import pytest

import mmtest as T
import surface as SF

pytestmark = pytest.mark.gpu

L, S, NFRAMES, ROWS = 5, 25.0, 5, 8
SHAPES = [(136, 20), (520, 24), (1040, 16), (1928, 12)]

# worst frame of each stream, oracle against float64 twin, both as codes:
# (max |difference|, share of values that differ).  CPU measurement, recorded.
TWIN_VS_ORACLE = {
    "synth 136x20": (1, 0.9e-4), "synth 520x24": (1, 1.8e-4), "synth 1040x16": (1, 2.7e-4),
    "synth 1928x12": (1, 2.9e-4), "saturating 1040x16": (1, 7.2e-4),
}   # (the worse of the two edge modes)


def _freeze(frames):
    for f in frames:
        f.setflags(write=False)
    return tuple(frames)


@functools.lru_cache(maxsize=None)
def _synth(W, H):
    return _freeze(T.synth(W, H, NFRAMES, fmt="u8"))


def saturating(W, H, n):
    """Channels of 0 and 255 in blocks (12, 16 and 20 columns by 4 rows) that
    move one to three columns a frame; alpha 255."""
    y, x = np.mgrid[0:H, 0:W]
    out = []
    for t in range(n):
        f = np.empty((H, W, 4), np.uint8)
        for c in range(3):
            f[..., c] = np.where(((x + t * (c + 1)) // (12 + 4 * c) + y // 4) % 2 == 0, 0, 255)
        f[..., 3] = 255
        out.append(f)
    return out


@functools.lru_cache(maxsize=None)
def _saturating(W, H):
    return _freeze(saturating(W, H, NFRAMES))


def _frames(kind, W, H):
    return list(_synth(W, H) if kind == "synth" else _saturating(W, H))


@functools.lru_cache(maxsize=None)
def _oracle(kind, W, H, edge):
    return _freeze(T.oracle_run(W, H, _frames(kind, W, H), L, S, edge))


def _gpu(kind, W, H, edge, mode, rows=None, oneshot=None):
    with SF.env(MM_K34_ROWS=rows, MM_K34_ONESHOT=oneshot):
        return T.gpu_run(W, H, _frames(kind, W, H), L, S, edge, mode=mode)


@functools.lru_cache(maxsize=None)
def _unfused(kind, W, H, edge, mode):
    return _freeze(_gpu(kind, W, H, edge, mode, rows="0"))


def _same(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), (what, k, int((x != y).sum()))


def _within_bar(got, kind, W, H, edge):
    ref = _oracle(kind, W, H, edge)
    assert np.array_equal(got[0], _frames(kind, W, H)[0]), "frame 0 passes through"
    worst = (0, 0.0)
    for g, r in zip(got[1:], ref[1:]):
        d = np.abs(g.astype(np.int32) - r.astype(np.int32))
        worst = max(worst, (int(d.max()), float((d > 0).mean())))
    print(f"{kind} {W}x{H} edge {edge}: worst frame vs oracle max {worst[0]} share {worst[1]:.2e}")
    for g, r in zip(got[1:], ref[1:]):
        T.assert_close_u8(g, r)


@pytest.mark.parametrize("mode", ["stream", "frame"])
@pytest.mark.parametrize("edge", [0, 1])
@pytest.mark.parametrize("W,H", SHAPES)
def test_three_forms_bitwise_and_oracle(W, H, edge, mode):
    """Fused strips, the one-shot form and the unfused pair write the same
    bytes, and those bytes are within the RGBA8 bar of the oracle."""
    unf = _unfused("synth", W, H, edge, mode)
    _same(_gpu("synth", W, H, edge, mode, rows=str(ROWS)), unf, "fused")
    _same(_gpu("synth", W, H, edge, mode, oneshot="2"), unf, "one-shot")
    _within_bar(unf, "synth", W, H, edge)


@pytest.mark.parametrize("mode", ["stream", "frame"])
@pytest.mark.parametrize("edge", [0, 1])
def test_register_loads_equal_staged_rows(edge, mode):
    """1040 x 16 from a surface with a pitch of 4164 bytes (4 mod 16): the
    launch keeps the register loads.  Same bytes as the packed stream's
    unfused pair, hence as its staged-row launch."""
    W, H, name = 1040, 16, "rgba8"
    fr = [np.ascontiguousarray(f).reshape(-1) for f in _synth(W, H)]
    lin = SF.lay_plus_unit(name, W, H)
    assert lin.pitch % 16 == 4
    with SF.env(MM_K34_ROWS=str(ROWS), MM_K34_ONESHOT=None):
        got = SF.run_pitched(name, W, H, fr, lin, SF.lay_tight(name, W, H), mode=mode,
                             params=SF.make_params(edge=edge))
    want = [f.reshape(-1) for f in _unfused("synth", W, H, edge, mode)]
    SF.assert_same(got, want, "register loads")


@pytest.mark.parametrize("edge", [0, 1])
def test_saturating_content(edge):
    """Both ends of the clamp: the input holds only 0 and 255, the output
    holds both, alpha stays 255, the three forms agree and the oracle's bar
    holds."""
    W, H, kind = 1040, 16, "saturating"
    assert set(np.unique(np.stack(_frames(kind, W, H)))) == {0, 255}
    unf = _unfused(kind, W, H, edge, "stream")
    _same(_gpu(kind, W, H, edge, "stream", rows=str(ROWS)), unf, "fused")
    _same(_gpu(kind, W, H, edge, "stream", oneshot="2"), unf, "one-shot")
    out = np.stack(unf[1:])
    assert (out[..., 3] == 255).all()
    for c in range(3):
        assert (out[..., c] == 0).any() and (out[..., c] == 255).any(), c
    _within_bar(unf, kind, W, H, edge)
