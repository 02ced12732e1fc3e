"""MM_MODE_STEERABLE's band kernels over the frequency sliders, the levels, the
canvas sizes and across mm_set_params, on the GPU.

k_sb_cols and k_sb_rows (csrc/mm_steer.hpp) decide per band and column from
(levels, min_freq, max_freq) what is transformed, stored and read back
(band_col_zero, the workgroup-uniform all_zero shortcut), and evaluate the
radial masks in fp32.  The rows of test_bands_host.CASES move the band edges
over the bins: bands that reach 0.5 (nothing skipped), bands skipped nearly
everywhere, inverted sliders, gaps, L = 2 (no middle band), the NaN band of
L = 3 and L = 7 with O = 8 (20 bands).  Everything is RGBA32F against the
float64 spec (oracle/steerable_ref.py) at test_steerable._close_spec's bars
(p99.9 < 2e-4, RMSE < 2e-5); the first frame is bitwise the input and every
output is finite.  tests/test_steer_bands_host.py shows that the spec alone
sits three orders of magnitude inside those bars at every row and that S moves
it by at least three times the bar.  Measured on an MI355X, worst frame:
p99.9 4.4e-7 / RMSE 7.1e-8 over the table (N = 128), 8.2e-7 / 1.5e-7 at
N = 512, 1.5e-6 / 2.8e-7 at N = 1024.
"""
import functools

import numpy as np
import pytest

from test_bands_host import CASES
from test_steer_bands_host import IDS, point
from test_steerable import SR, _close_spec, frames, gpu_steer

pytestmark = pytest.mark.gpu

ANCHORS = [(5, 0.05, 0.45), (6, 0.05, 0.45)]


def row_id(r):
    return f"L{r[0]}-{r[1]:g}-{r[2]:g}"


@functools.lru_cache(maxsize=None)
def _frames(W, H, n):
    fr = tuple(frames(W, H, n))
    for f in fr:
        f.flags.writeable = False
    return fr


def _black(W, H):
    f = np.zeros((H, W, 4), np.float32)
    f[..., 3] = 1.0
    return f


def _spec(fr, W, H, L, minf, maxf, S, Oo, filt, edge=0, tau=0.01, rl=0.05, rh=0.4):
    r = SR.SteerableRef(W, H, levels=L, min_freq=minf, max_freq=maxf, phase_scale=S, orientations=Oo,
                        filt=filt, r_low=rl, r_high=rh, tau=tau, edge=edge)
    return [r.process(f.astype(np.float64)) for f in fr]


def _check(got, fr, ref, what, first=1):
    """Frames [first, n) against the spec; frame 0 passes through bitwise."""
    got = np.asarray(got)
    assert np.isfinite(got).all(), what
    if first:
        assert np.array_equal(got[0], fr[0]), "the first frame passes through bitwise"
    for k in range(first, len(fr)):
        e = np.abs(got[k].astype(np.float64) - ref[k])
        print(f"{what} frame {k}: max {e.max():.3g} p99.9 {np.quantile(e, 0.999):.3g} "
              f"rmse {np.sqrt((e ** 2).mean()):.3g}")
    for k in range(first, len(fr)):
        _close_spec(got[k], ref[k])
        assert np.all(got[k][..., 3] == 1.0)


def _params(L, minf, maxf, S, Oo, filt, edge=0, tau=0.01, rl=0.05, rh=0.4):
    import mm355
    return mm355.Params.make(levels=L, min_freq=minf, max_freq=maxf, phase_scale=S,
                             magnitude_threshold=tau, edge_mode=edge, mode=mm355.MODE_STEERABLE,
                             orientations=Oo, temporal_filter=filt, iir_low=rl, iir_high=rh)


def _by_frame(W, H, fr, params, batch, want_state=False):
    """One mm_process call per frame; optionally the final state planes (floats)."""
    import mm355
    import torch
    h = mm355.Handle(W, H, params)
    h.set_batch(batch)
    dev = torch.from_numpy(np.stack(fr)).cuda()
    out = torch.empty_like(dev)
    for k in range(len(fr)):
        h.process(dev[k], out[k], mm355.RGBA32F)
    st = None
    if want_state:
        buf = torch.empty(h.state_bytes, dtype=torch.uint8, device="cuda")
        h.get_state(buf)
        torch.cuda.synchronize()
        st = buf.cpu().numpy().view(np.float32)
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    h.close()
    return (res, st) if want_state else res


# ---- a. every row of the table, N = 128 ---------------------------------------------
@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_table(k):
    """4 frames at batch 3 (one batch boundary); orientations, filter and edge
    mode walk over the rows (test_steer_bands_host.point); S = 25 on even rows,
    9.7 on odd ones.  The same frames in one-frame mm_process calls are
    bitwise the stream's."""
    L, minf, maxf, _ = CASES[k]
    Oo, filt, edge = point(k)
    S = 9.7 if k & 1 else 25.0
    W, H, n = 96, 64, 4
    fr = _frames(W, H, n)
    got = gpu_steer(W, H, fr, levels=L, S=S, Oo=Oo, filt=filt, edge=edge, batch=3, minf=minf, maxf=maxf)
    ref = _spec(fr, W, H, L, minf, maxf, S, Oo, filt, edge)
    _check(got, fr, ref, f"{IDS[k]} O={Oo} filt={filt} S={S:g}")
    one = _by_frame(W, H, fr, _params(L, minf, maxf, S, Oo, filt, edge), 3)
    assert np.array_equal(one, got)


# ---- b. portrait and odd sizes ------------------------------------------------------
SIX = ANCHORS + [(4, 0.05, 0.10), (5, 0.45, 0.10), (7, 0.02, 0.60), (5, 0.45, 0.50)]


@pytest.mark.parametrize("W,H", [(63, 95), (64, 96)])
@pytest.mark.parametrize("i", range(len(SIX)), ids=[row_id(r) for r in SIX])
def test_portrait(i, W, H):
    """H > W: the canvas is sized by the rows, the column offset x0 is the
    large one (63 x 95: both offsets fractional, k_compose_odd)."""
    L, minf, maxf = SIX[i]
    filt, Oo, edge, n = i & 1, (8, 6, 4)[i % 3], W & 1, 4
    fr = _frames(W, H, n)
    got = gpu_steer(W, H, fr, levels=L, S=25.0, Oo=Oo, filt=filt, edge=edge, minf=minf, maxf=maxf)
    _check(got, fr, _spec(fr, W, H, L, minf, maxf, 25.0, Oo, filt, edge), f"{W}x{H} {row_id(SIX[i])}")


# ---- c. the N = 512 and N = 1024 instances ------------------------------------------
# Three frames of the float64 spec take ~1.4 s (N = 512) and ~7 s (N = 1024) on
# one CPU thread, which the timeout is sized for; the GPU part is milliseconds.
@pytest.mark.timeout(300)
@pytest.mark.parametrize("filt", [0, 1])
@pytest.mark.parametrize("row", [(5, 0.05, 0.45), (6, 0.05, 0.30), (4, 0.05, 0.50), (5, 0.45, 0.10)],
                         ids=row_id)
@pytest.mark.parametrize("W,H", [(300, 24), (24, 300), (520, 40)])
def test_transform_sizes(W, H, row, filt):
    """k_cols_fwd, k_sb_cols and k_sb_rows at LOG2N = 9 and 10 (24 x 300:
    portrait, x0 = 244)."""
    L, minf, maxf = row
    n = 3
    fr = _frames(W, H, n)
    got = gpu_steer(W, H, fr, levels=L, S=25.0, Oo=8, filt=filt, minf=minf, maxf=maxf)
    _check(got, fr, _spec(fr, W, H, L, minf, maxf, 25.0, 8, filt), f"{W}x{H} {row_id(row)} filt={filt}")


# ---- d. the threshold and the IIR coefficients ----------------------------------------
# tau = 0 gates nothing; tau = 0.5 gates most coefficients (s' = s, the state
# still follows the input).  iir_high = 1 makes u_h identically 0.  Six frames:
# the filter memory matters.
@pytest.mark.parametrize("filt,rl,rh", [(0, 0.05, 0.4), (1, 0.01, 1.0), (1, 0.2, 0.21), (1, 0.05, 0.4)])
@pytest.mark.parametrize("tau", [0.0, 0.5])
@pytest.mark.parametrize("row", [(5, 0.05, 0.45), (6, 0.05, 0.30)], ids=row_id)
def test_threshold_and_iir(row, tau, filt, rl, rh):
    L, minf, maxf = row
    W, H, n = 96, 64, 6
    fr = _frames(W, H, n)
    got = gpu_steer(W, H, fr, levels=L, S=25.0, Oo=8, filt=filt, rl=rl, rh=rh, minf=minf, maxf=maxf,
                    tau=tau)
    ref = _spec(fr, W, H, L, minf, maxf, 25.0, 8, filt, tau=tau, rl=rl, rh=rh)
    _check(got, fr, ref, f"{row_id(row)} tau={tau:g} filt={filt} r=({rl:g}, {rh:g})")


# ---- e. black frames --------------------------------------------------------------------
def _black_stream(which, W, H):
    s, b = _frames(W, H, 5), _black(W, H)
    return [s[0], b, s[2], s[3], s[4]] if which == "mid" else [b, b, s[2], s[3]]


@pytest.mark.parametrize("row", [(5, 0.05, 0.45), (5, 0.45, 0.50)], ids=row_id)
@pytest.mark.parametrize("tau", [0.0, 0.01])
@pytest.mark.parametrize("filt", [0, 1])
@pytest.mark.parametrize("which", ["mid", "lead"])
def test_black_frames(which, filt, tau, row):
    """Every band coefficient of a black frame is exactly zero, and its phase
    goes into the state: arctan2(0, 0) = 0 in the spec
    (test_steer_bands_host.test_spec_black_frame_phase_is_zero), so
    fast_atan2_x2 must give 0 there, not NaN.  Under IIR the state carries it
    into every later frame.  The black frame comes out black; the state read
    back after the stream is finite."""
    L, minf, maxf = row
    W, H = 96, 64
    fr = _black_stream(which, W, H)
    ref = _spec(fr, W, H, L, minf, maxf, 25.0, 8, filt, tau=tau)
    got = gpu_steer(W, H, fr, levels=L, S=25.0, Oo=8, filt=filt, minf=minf, maxf=maxf, tau=tau, batch=3)
    what = f"{which} {row_id(row)} tau={tau:g} filt={filt}"
    _check(got, fr, ref, what)
    for k in ((1,) if which == "mid" else (0, 1)):
        assert np.all(got[k][..., :3] == 0) and np.all(got[k][..., 3] == 1), k
    one, st = _by_frame(W, H, fr, _params(L, minf, maxf, 25.0, 8, filt, tau=tau), 3, want_state=True)
    assert np.array_equal(one, got)
    # phi (and u_h, u_l under IIR) of (L - 2) O / 2 bands, W + 4 columns per row
    assert st.size > 0 and st.size % ((1 + 2 * filt) * (L - 2) * 4 * (W + 4)) == 0
    assert np.isfinite(st).all(), what


# ---- f. mm_set_params in steerable mode ------------------------------------------------
# Three frames per stage.  A stage whose change clears the local-phase state
# restarts the stream: its first frame passes through and its outputs are a
# fresh handle's, bitwise.  A phase_scale-only or magnitude_threshold-only
# change keeps the state: no frame passes through and the outputs follow the
# spec that ran on from the last restart with its S / tau changed at that frame.
RW, RH, RPER = 63, 47, 3
# tau = 0.001: at 0.01 this small canvas has every coefficient gated in stages
# 1 to 4 and S would move nothing there.
RBASE = dict(L=5, minf=0.05, maxf=0.45, S=10.0, Oo=8, tau=0.001, rl=0.05, rh=0.4)
RSTAGES = [
    ({}, True),                          # 0 the stream's start
    (dict(minf=0.06), True),             # 1 min_freq
    (dict(maxf=0.40), True),             # 2 max_freq
    (dict(L=7), True),                   # 3 levels: 12 -> 20 bands
    (dict(L=4), True),                   # 4 levels: 20 -> 8 bands
    (dict(Oo=4), True),                  # 5 orientations: 8 -> 4 bands
    (dict(rl=0.10), True),               # 6 iir_low
    (dict(rh=0.60), True),               # 7 iir_high
    (dict(S=25.0), False),               # 8 phase_scale only
    (dict(tau=0.5), False),              # 9 magnitude_threshold only
]


def _reload_stages():
    cur, out = dict(RBASE), []
    for ch, clears in RSTAGES:
        cur = dict(cur, **ch)
        out.append((dict(cur), clears))
    return out


@pytest.mark.parametrize("filt", [0, 1])
def test_hot_reload(filt):
    import mm355
    import torch
    stages = _reload_stages()
    n = RPER * len(stages)
    fr = _frames(RW, RH, n)
    dev = torch.from_numpy(np.stack(fr)).cuda()

    def params(s):
        return _params(s["L"], s["minf"], s["maxf"], s["S"], s["Oo"], filt, tau=s["tau"], rl=s["rl"],
                       rh=s["rh"])

    h = mm355.Handle(RW, RH, params(stages[0][0]))
    h.set_batch(2)                       # every stage crosses a batch boundary
    out = torch.empty_like(dev)
    fresh = torch.zeros_like(dev)
    for i, (s, clears) in enumerate(stages):
        a, b = RPER * i, RPER * (i + 1)
        if i:
            h.set_params(params(s))
        h.process_stream(dev[a:b], out[a:b], RPER, mm355.RGBA32F)
        if clears:
            g = mm355.Handle(RW, RH, params(s))
            g.set_batch(2)
            g.process_stream(dev[a:b], fresh[a:b], RPER, mm355.RGBA32F)
            torch.cuda.synchronize()
            g.close()
    torch.cuda.synchronize()
    got, fresh = out.cpu().numpy(), fresh.cpu().numpy()
    h.close()
    assert np.isfinite(got).all()

    ref = None
    for i, (s, clears) in enumerate(stages):
        a, b = RPER * i, RPER * (i + 1)
        if clears:
            assert np.array_equal(got[a], fr[a]), f"stage {i}: the frame after the change passes through"
            assert np.array_equal(got[a:b], fresh[a:b]), f"stage {i}: a fresh handle's outputs"
            ref = SR.SteerableRef(RW, RH, levels=s["L"], min_freq=s["minf"], max_freq=s["maxf"],
                                  phase_scale=s["S"], orientations=s["Oo"], filt=filt, r_low=s["rl"],
                                  r_high=s["rh"], tau=s["tau"])
            stale = None
        else:
            # the spec that did not hear of the change, from the same state
            stale = SR.SteerableRef(RW, RH, levels=s["L"], min_freq=s["minf"], max_freq=s["maxf"],
                                    phase_scale=ref.S, orientations=s["Oo"], filt=filt, r_low=s["rl"],
                                    r_high=s["rh"], tau=ref.tau)
            stale.state = ref.state
            ref.S, ref.tau = s["S"], s["tau"]
        rs = [ref.process(f.astype(np.float64)) for f in fr[a:b]]
        if clears:
            _check(got[a:b], fr[a:b], rs, f"stage {i} filt={filt}")
            # the stage magnifies something: S moves its last frame by three times the bar
            still = SR.SteerableRef(RW, RH, levels=s["L"], min_freq=s["minf"], max_freq=s["maxf"],
                                    phase_scale=0.0, orientations=s["Oo"], filt=filt, r_low=s["rl"],
                                    r_high=s["rh"], tau=s["tau"])
            s0 = [still.process(f.astype(np.float64)) for f in fr[a:b]]
            assert np.quantile(np.abs(s0[-1] - rs[-1]), 0.999) >= 6e-4, f"stage {i} magnifies too little"
        else:
            for k in range(a, b):
                assert not np.array_equal(got[k], fr[k]), f"stage {i}: frame {k} passed through"
            _check(got[a:b], fr[a:b], rs, f"stage {i} filt={filt}", first=0)
            # the change moves the spec by three times the bar: a kept old
            # value cannot hide inside it
            so = stale.process(fr[a].astype(np.float64))
            assert np.quantile(np.abs(so - rs[0]), 0.999) >= 6e-4, f"stage {i} changes too little"
