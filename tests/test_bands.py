"""K2's band paths over the frequency sliders and across mm_set_params, on the GPU.

The rows of test_bands_host.CASES put (levels, min_freq, max_freq) into each
of K2's three band classes at several values of levels (TAB: one-band op from
the table; TAB2: per-wave one-/two-band op with the mask-sum array; GENERIC:
masks per bin and frame), with gaps, inverted sliders, coinciding bands and
low-pass / high-pass shoulders that reach the middle bands.  Everything here
is judged against the CPU oracle at the project's bars (mmtest.TOL_*, integer
phase scales unless said), which test_bands_host.py pins against the float64
twin at the same rows.
"""
import functools

import numpy as np
import pytest

import mmtest as T
import nv12
import oracle_py as O
from test_bands_host import CASES, GENERIC, TAB, TAB2, case_id

pytestmark = pytest.mark.gpu

SCALES = (25.0, 10.0, -25.0)
# one row per class, off the defaults
ROW = {TAB: (5, 0.05, 0.50), TAB2: (5, 0.05, 0.30), GENERIC: (6, 0.10, 0.20)}
PER_CLASS = [ROW[TAB], ROW[TAB2], ROW[GENERIC]]


def row_id(r):
    return f"L{r[0]}-{r[1]:g}-{r[2]:g}"


@functools.lru_cache(maxsize=None)
def _frames(W, H, n, fmt="f32"):
    fr = T.synth(W, H, n, fmt=fmt)
    for f in fr:
        f.flags.writeable = False
    return tuple(fr)


def _oracle(W, H, frames, L, minf, maxf, S, edge=0, tau=0.01):
    o = O.Oracle(W, H, levels=L, min_freq=minf, max_freq=maxf, phase_scale=S, mag_threshold=tau,
                 edge_mode=edge)
    out = [o.process(f) for f in frames]
    o.close()
    for r in out:
        r.flags.writeable = False
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _ref(W, H, n, L, minf, maxf, S, edge=0, tau=0.01, fmt="f32"):
    """The oracle's outputs, computed once per case and shared."""
    if W >= 1024:
        O.set_threads(16)
    return _oracle(W, H, _frames(W, H, n, fmt), L, minf, maxf, S, edge, tau)


def _close(got, ref, what, integer=True):
    mx, rmse, p999 = T.err_stats(got, ref)
    print(f"{what}: max {mx:.3g} rmse {rmse:.3g} p99.9 {p999:.3g}")
    T.assert_close_f32(got, ref, integer_scale=integer)


def _check_f32(got, fr, ref, what, integer=True):
    assert np.array_equal(got[0], fr[0]), "first frame passes through bitwise"
    for k in range(1, len(fr)):
        _close(got[k], ref[k], f"{what} frame {k}", integer)
        assert np.all(got[k][..., 3] == 1.0)


def _run(W, H, n, L, minf, maxf, S, edge=0, tau=0.01, **kw):
    return T.gpu_run(W, H, list(_frames(W, H, n)), L, S, edge, minf=minf, maxf=maxf,
                     extra=dict(magnitude_threshold=tau), **kw)


# ---- 1. every row, N = 64 --------------------------------------------------------
def _sweep_point(k):
    return SCALES[k % 3], k & 1          # all six (S, edge) pairs occur over the rows


@pytest.mark.parametrize("k", range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_sweep(k):
    L, minf, maxf, _ = CASES[k]
    S, edge = _sweep_point(k)
    W, H, n = 64, 48, 4
    got = _run(W, H, n, L, minf, maxf, S, edge)
    _check_f32(got, _frames(W, H, n), _ref(W, H, n, L, minf, maxf, S, edge), case_id(CASES[k]))


@pytest.mark.parametrize("row", PER_CLASS, ids=row_id)
def test_non_integer_scale(row):
    """S = 9.7: wrap ties at |delta| ~ pi leave the max unbounded, so the
    99.9th percentile bar (mmtest.assert_close_f32, integer_scale=False)."""
    W, H, n = 64, 48, 4
    got = _run(W, H, n, *row, 9.7)
    _check_f32(got, _frames(W, H, n), _ref(W, H, n, *row, 9.7), row_id(row), integer=False)


# ---- 2. other launch shapes: the one-band / two-band wave split moves with N ----------
@pytest.mark.parametrize("W,H,n,row", [
    # N = 256, eight columns per workgroup
    (200, 120, 4, (4, 0.05, 0.50)), (200, 120, 4, (4, 0.20, 0.45)), (200, 120, 4, (5, 0.10, 0.20)),
    # odd sizes, N = 128: K1's generic taps, k_compose_odd
    (95, 63, 4, (5, 0.05, 0.50)), (95, 63, 4, (5, 0.15, 0.50)), (95, 63, 4, (6, 0.20, 0.45)),
    # N = 2048, two columns per workgroup
    (1100, 16, 3, (6, 0.02, 0.60)), (1100, 16, 3, (7, 0.05, 0.50)), (1100, 16, 3, (6, 0.10, 0.20)),
], ids=lambda v: row_id(v) if isinstance(v, tuple) else str(v))
def test_other_sizes(W, H, n, row):
    S, edge = (25.0, 0) if W != 95 else (-25.0, 1)
    got = _run(W, H, n, *row, S, edge)
    _check_f32(got, _frames(W, H, n), _ref(W, H, n, *row, S, edge), f"{W}x{H} {row_id(row)}")


# ---- 3. k_cols_tail and the second-half tail blocks (batches of >= 24 frames) ---------
@pytest.mark.parametrize("row", [ROW[TAB2], ROW[GENERIC]], ids=row_id)
@pytest.mark.parametrize("W,H", [(64, 48), (200, 120)])
def test_tails(W, H, row):
    n = 26
    st = _run(W, H, n, *row, 25.0, mode="stream", batch=26)
    _check_f32(st, _frames(W, H, n), _ref(W, H, n, *row, 25.0), f"{W}x{H} {row_id(row)}")
    fm = _run(W, H, n, *row, 25.0, mode="frame", batch=1)
    for k in range(n):
        assert np.array_equal(st[k], fm[k]), k


# ---- 4. formats: the masks are format-blind ---------------------------------------
@pytest.mark.parametrize("row", [ROW[TAB2], ROW[GENERIC]], ids=row_id)
def test_rgba8(row):
    W, H, n = 200, 120, 4
    fr = _frames(W, H, n, "u8")
    ref = _ref(W, H, n, *row, 25.0, fmt="u8")
    L, minf, maxf = row
    got = T.gpu_run(W, H, list(fr), L, 25.0, minf=minf, maxf=maxf)
    assert np.array_equal(got[0], fr[0])
    for k in range(1, n):
        T.assert_close_u8(got[k], ref[k])


@pytest.mark.parametrize("row", [ROW[TAB2], ROW[GENERIC]], ids=row_id)
def test_nv12(row):
    """An NV12 frame is the RGBA32F frame of its BT.601 decode (tests/nv12.py)."""
    import mm355
    W, H, n = 200, 120, 4
    L, minf, maxf = row
    fr = [nv12.encode(f) for f in _frames(W, H, n, "u8")]
    ref = [nv12.encode(r) for r in
           _oracle(W, H, [nv12.decode(b, np.float32) for b in fr], L, minf, maxf, 25.0)]
    got = T.gpu_run(W, H, fr, L, 25.0, minf=minf, maxf=maxf, batch=1, fmt=mm355.NV12)
    assert np.array_equal(got[0], fr[0])
    for k in range(1, n):
        T.assert_close_u8(got[k], ref[k])
        assert (got[k][:H] != fr[k][:H]).mean() > 0.5      # not a passthrough


# ---- 5. the table path and the per-bin path at every table point -------------------
NOTAB = [k for k, c in enumerate(CASES) if c[3] in (TAB, TAB2)]


@pytest.mark.parametrize("k", NOTAB, ids=[case_id(CASES[k]) for k in NOTAB])
def test_generic_twin(k, monkeypatch):
    """MM_K2_NOTAB=1 (read when the handle is made) runs K2's generic per-bin
    op on the layouts the tables serve: same oracle output, same bar."""
    monkeypatch.setenv("MM_K2_NOTAB", "1")
    L, minf, maxf, _ = CASES[k]
    S, edge = _sweep_point(k)
    W, H, n = 64, 48, 4
    got = _run(W, H, n, L, minf, maxf, S, edge)
    _check_f32(got, _frames(W, H, n), _ref(W, H, n, L, minf, maxf, S, edge), case_id(CASES[k]))


# ---- 6. mm_set_params mid-stream ---------------------------------------------------
# edge_mode stays fixed (its mid-stream change is a documented divergence,
# include/mm.h mm_set_params).  Each step holds for three frames (the last for
# two): nine steps, 26 frames.  The last step's tau = 0.5 moves the oracle's
# output by 6e-4, six times the bar; one gate decision that differs between
# the GPU and the oracle moves a pixel by at most 2 tau / N^2 = 1.5e-5.
RELOAD_W, RELOAD_H, RELOAD_N = 200, 120, 26
RELOAD_STEPS = [
    dict(L=5, minf=0.05, maxf=0.45),                          # 1 TAB, the default
    dict(L=5, minf=0.05, maxf=0.50),                          # 2 TAB again: the table is rebuilt all the same
    dict(L=5, minf=0.05, maxf=0.30),                          # 3 TAB2
    dict(L=6, minf=0.05, maxf=0.30),                          # 4 TAB2, other levels
    dict(L=6, minf=0.10, maxf=0.20),                          # 5 GENERIC
    dict(L=6, minf=0.10, maxf=0.20, std=True),                # 6 standard mode
    dict(L=5, minf=0.15, maxf=0.50),                          # 7 TAB2
    dict(L=5, minf=0.15, maxf=0.50, S=10.0),                  # 8 phase_scale only
    dict(L=5, minf=0.15, maxf=0.50, S=10.0, tau=0.5),         # 9 magnitude_threshold only
]


def _step_of(k):
    return min(k // 3, len(RELOAD_STEPS) - 1)


@functools.lru_cache(maxsize=None)
def _reload_ref():
    fr = _frames(RELOAD_W, RELOAD_H, RELOAD_N)
    o = O.Oracle(RELOAD_W, RELOAD_H)
    out, cur = [], -1
    for k, f in enumerate(fr):
        if _step_of(k) != cur:
            cur = _step_of(k)
            s = RELOAD_STEPS[cur]
            o.set_params(s["L"], s["minf"], s["maxf"], s.get("S", 25.0), s.get("tau", 0.01))
            o.set_standard(s.get("std", False))
        out.append(o.process(f))
    o.close()
    return tuple(out)


def _reload_gpu(how):
    """how: "frame" (one mm_process per frame), "stream2" (each step's frames in
    one mm_process_stream call on a batch-2 handle: every call crosses a batch
    boundary) or "stream8" (batch 8: a call is one launch)."""
    import mm355
    import torch
    W, H = RELOAD_W, RELOAD_H

    def params(s):
        kw = dict(mode=mm355.MODE_STANDARD, **T._std_fields({})) if s.get("std") else {}
        return mm355.Params.make(levels=s["L"], min_freq=s["minf"], max_freq=s["maxf"],
                                 phase_scale=s.get("S", 25.0), magnitude_threshold=s.get("tau", 0.01),
                                 **kw)

    dev_in = torch.from_numpy(np.stack(_frames(W, H, RELOAD_N))).cuda()
    dev_out = torch.empty_like(dev_in)
    h = mm355.Handle(W, H, params(RELOAD_STEPS[0]))
    h.set_batch(2 if how == "stream2" else 8)
    for i, s in enumerate(RELOAD_STEPS):
        ks = [k for k in range(RELOAD_N) if _step_of(k) == i]
        if i:
            h.set_params(params(s))
        if how == "frame":
            for k in ks:
                h.process(dev_in[k], dev_out[k], mm355.RGBA32F)
        else:
            h.process_stream(dev_in[ks[0]:ks[-1] + 1], dev_out[ks[0]:ks[-1] + 1], len(ks), mm355.RGBA32F)
    torch.cuda.synchronize()
    res = dev_out.cpu().numpy()
    h.close()
    return res


def test_hot_reload():
    """One handle and one oracle walk RELOAD_STEPS; the state is kept across
    mm_set_params, so every frame after the first is a magnified one and meets
    the bar.  A table (d_ktab / d_kmsum) left from the step before would miss
    it from that step on."""
    fr, ref = _frames(RELOAD_W, RELOAD_H, RELOAD_N), _reload_ref()
    got = _reload_gpu("frame")
    # the steps do move the output: a stale table cannot hide inside the bar
    for i in range(1, len(RELOAD_STEPS)):
        k = 3 * i
        o = O.Oracle(RELOAD_W, RELOAD_H)
        s = RELOAD_STEPS[i - 1]
        o.set_params(s["L"], s["minf"], s["maxf"], s.get("S", 25.0), s.get("tau", 0.01))
        o.set_standard(s.get("std", False))
        o.process(fr[k - 1])
        assert np.abs(o.process(fr[k]) - ref[k]).max() > 5 * T.TOL_MAX, f"step {i + 1} changes nothing"
        o.close()
    assert np.array_equal(got[0], fr[0])
    for k in range(1, RELOAD_N):
        _close(got[k], ref[k], f"step {_step_of(k) + 1} frame {k}")
    for how in ("stream2", "stream8"):
        other = _reload_gpu(how)
        for k in range(RELOAD_N):
            assert np.array_equal(got[k], other[k]), (how, k)


# ---- 7. the magnitude threshold ----------------------------------------------------
# N = 256: one gate decision that differs between the GPU and the oracle moves
# a pixel by at most 2 tau / N^2 = 3e-6 at tau = 0.1, well inside the bar.
@pytest.mark.parametrize("tau", [0.001, 0.1])
@pytest.mark.parametrize("row", PER_CLASS, ids=row_id)
def test_threshold(row, tau):
    W, H, n = 200, 120, 3
    got = _run(W, H, n, *row, 25.0, tau=tau)
    _check_f32(got, _frames(W, H, n), _ref(W, H, n, *row, 25.0, tau=tau), f"tau {tau} {row_id(row)}")


@pytest.mark.parametrize("row", PER_CLASS, ids=row_id)
def test_threshold_gates_everything(row):
    """tau = 1e6 gates every middle bin: the phase scale has no effect, bitwise."""
    W, H, n = 200, 120, 3
    got = _run(W, H, n, *row, 25.0, tau=1e6)
    still = _run(W, H, n, *row, 0.0, tau=1e6)
    for k in range(n):
        assert np.array_equal(got[k], still[k]), k
    _check_f32(got, _frames(W, H, n), _ref(W, H, n, *row, 25.0, tau=1e6), f"tau 1e6 {row_id(row)}")


# ---- 8. exact-zero bins at tau = 0 --------------------------------------------------
def _black(W, H, dtype):
    f = np.zeros((H, W, 4), dtype)
    f[..., 3] = 255 if dtype == np.uint8 else 1.0
    return f


# (4100 x 16: N = 8192, where overlapping bands have no two-band instance)
@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("W,H,row", [(64, 48, ROW[TAB]), (64, 48, ROW[TAB2]), (64, 48, ROW[GENERIC]),
                                     (64, 48, (5, 0.05, 0.45)), (4100, 16, (6, 0.05, 0.45))],
                         ids=lambda v: row_id(v) if isinstance(v, tuple) else str(v))
def test_black_frames_at_zero_threshold(W, H, row, dtype):
    """A black frame's spectrum is exactly zero and tau = 0 gates nothing, so
    every magnified bin takes the phase of (0, 0): the reference's atan2(0, 0)
    is 0 and A = c w = 0.  The output is black, not NaN.  (The compose stage
    saturates, which turns a NaN luma into 0 as well: on black frames alone a
    NaN in K2 does not show.  test_black_synth_black_at_zero_threshold is the
    one that sees it.)"""
    L, minf, maxf = row
    fr = [_black(W, H, dtype)] * 2
    got = T.gpu_run(W, H, fr, L, 25.0, minf=minf, maxf=maxf, extra=dict(magnitude_threshold=0.0))
    assert np.array_equal(got[0], fr[0])
    assert np.isfinite(got[1]).all()
    assert np.all(got[1][..., :3] == 0)
    assert np.all(got[1][..., 3] == fr[0][..., 3])


@pytest.mark.parametrize("row", PER_CLASS + [(5, 0.05, 0.45)], ids=row_id)
def test_black_synth_black_at_zero_threshold(row):
    """black -> synth -> black at tau = 0.  Frame 1 pairs a nonzero c with an
    exactly zero p: the reference takes arg p - arg c with atan2(0, 0) = 0, so
    delta = -arg c there (not 0, the phase of p conj c = 0).  Frame 2 has
    c = 0: A = 0.  Before K2 ran its generic op at thresholds that gate no
    zero bin, the table paths gave max errors of 0.81 (TAB rows: atan2_nz's
    0 * rcp(0) = NaN at bin (N/2, 0), over the whole frame and saturated to
    black), 0.074 (TAB2) and 0.042 (GENERIC) on frame 1."""
    W, H = 64, 48
    L, minf, maxf = row
    fr = [_black(W, H, np.float32), _frames(W, H, 2)[1], _black(W, H, np.float32)]
    ref = _oracle(W, H, fr, L, minf, maxf, 25.0, tau=0.0)
    got = T.gpu_run(W, H, fr, L, 25.0, minf=minf, maxf=maxf, extra=dict(magnitude_threshold=0.0))
    assert np.isfinite(np.stack(got)).all()
    _check_f32(got, fr, ref, f"black-synth-black {row_id(row)}")
