"""MM_MODE_STEERABLE's band logic over the frequency sliders, host side (no GPU).

csrc/mm_steer.hpp decides from (levels, min_freq, max_freq) which columns of
which band are identically zero (band_col_zero: k_sb_cols skips them,
k_sb_rows reads zeros for them) and evaluates the radial masks in fp32
(level_mask).  tests/test_steer_bands.py runs the rows of
test_bands_host.CASES through those kernels against the float64 spec
(oracle/steerable_ref.py).  This file keeps that table honest for the
steerable mode (the class column is K2's and is ignored here):

  - the spec at S = 0 is the reference pipeline at every row, so its masks are
    the reference's over the whole table, not only at the defaults;
  - the spec is well conditioned at every row: an input perturbation of one
    fp32 ulp moves it by a thousandth of the GPU bars, so a GPU miss is about
    the kernels, not about a wrap tie in the content;
  - the spec's S = 25 output is far from its S = 0 output at every row with a
    middle band, so a band that the kernels drop cannot hide inside the bars;
  - a float32 restatement of band_col_zero shows the table reaching every kind
    of skip pattern (none, nearly all, inverted order, L = 7).
"""
import functools

import numpy as np
import pytest

import np_twin
import oracle_py as O
from test_bands_host import CASES, band_edges_f32, case_id
from test_steerable import SR, frames

IDS = [case_id(c) for c in CASES]


def point(k):
    """Orientations, temporal filter and edge mode of table row k (shared with
    tests/test_steer_bands.py)."""
    return (4, 6, 8)[k % 3], k & 1, k & 1


@functools.lru_cache(maxsize=None)
def frames64(W, H, n):
    fr = tuple(f.astype(np.float64) for f in frames(W, H, n))
    for f in fr:
        f.flags.writeable = False
    return fr


def spec_run(fr, W, H, L, minf, maxf, S, Oo, filt, edge=0, **kw):
    r = SR.SteerableRef(W, H, levels=L, min_freq=minf, max_freq=maxf, phase_scale=S, orientations=Oo,
                        filt=filt, edge=edge, **kw)
    return [r.process(np.asarray(f, np.float64)) for f in fr]


def stats(a, b):
    e = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return float(e.max()), float(np.quantile(e, 0.999)), float(np.sqrt((e ** 2).mean()))


# ---- 1. the spec over the table at S = 0 ----------------------------------------
@pytest.mark.parametrize("filt", [SR.FILTER_DIFF, SR.FILTER_IIR])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_spec_s0_is_reference_pipeline_over_table(case, filt):
    """sum_o a_o = 1 on every bin, so at S = 0 the spec is the reference
    pipeline at the row's sliders: the float64 twin to 1e-12
    (test_steerable.test_spec_s0_is_reference_pipeline's reference and bar),
    and the C oracle, whose frames are fp32, at the bars that pin it to the
    twin (test_bands_host._oracle_vs_twin: max 5e-6, RMSE 1e-6)."""
    L, minf, maxf, _ = case
    W, H = 64, 48
    fr = frames64(W, H, 3)
    outs = spec_run(fr, W, H, L, minf, maxf, 0.0, 8, filt)
    assert np.array_equal(outs[0], fr[0])
    ref = np_twin.process_frame(fr[2], fr[1], L, minf, maxf, 0.0)
    assert np.abs(outs[2] - ref).max() < 1e-12
    o = O.Oracle(W, H, levels=L, min_freq=minf, max_freq=maxf, phase_scale=0.0)
    for f in fr[:2]:
        o.process(f.astype(np.float32))
    c = o.process(fr[2].astype(np.float32))
    o.close()
    mx, _, rmse = stats(outs[2], c)
    print(f"S=0 spec vs C oracle: max {mx:.3g} rmse {rmse:.3g}")
    assert mx < 5e-6 and rmse < 1e-6, (mx, rmse)


# ---- 2. conditioning ---------------------------------------------------------------
CW, CH, CN = 96, 64, 4


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_spec_conditioning(k):
    """The spec on the frames and on the frames times (1 + u 2^-23): a tenth
    of _close_spec's bars (p99.9 2e-5, RMSE 2e-6) on every non-first frame.
    Measured: max-abs <= 2.4e-7 at every row, both filters."""
    L, minf, maxf, _ = CASES[k]
    Oo, filt, edge = point(k)
    fr = frames64(CW, CH, CN)
    rng = np.random.default_rng(1000 + k)
    fr2 = [f * (1.0 + rng.uniform(-1.0, 1.0, f.shape) * 2.0 ** -23) for f in fr]
    a = spec_run(fr, CW, CH, L, minf, maxf, 25.0, Oo, filt, edge)
    b = spec_run(fr2, CW, CH, L, minf, maxf, 25.0, Oo, filt, edge)
    for t in range(1, CN):
        mx, p999, rmse = stats(a[t], b[t])
        print(f"{IDS[k]} O={Oo} filt={filt} frame {t}: max {mx:.3g} p99.9 {p999:.3g} rmse {rmse:.3g}")
        assert p999 <= 2e-5 and rmse <= 2e-6, (t, mx, p999, rmse)


# ---- 3. power ----------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_spec_power(k):
    """O = 8, DIFF: the last frame at S = 25 is at least 6e-4 (p99.9, three
    times the GPU bar) from the S = 0 frame at every row with L >= 4 (measured
    minimum 7.2e-4 at (5, 0.15, 0.50), edge mode 0); at L = 2 and L = 3 no band carries
    anything and the two are equal."""
    L, minf, maxf, _ = CASES[k]
    fr = frames64(CW, CH, CN)
    a = spec_run(fr, CW, CH, L, minf, maxf, 25.0, 8, SR.FILTER_DIFF)[-1]
    b = spec_run(fr, CW, CH, L, minf, maxf, 0.0, 8, SR.FILTER_DIFF)[-1]
    mx, p999, rmse = stats(a, b)
    print(f"{IDS[k]}: S=25 vs S=0 max {mx:.3g} p99.9 {p999:.3g} rmse {rmse:.3g}")
    if L >= 4:
        assert p999 >= 6e-4, p999
    else:
        assert mx == 0.0, mx


# ---- 4. the skip pattern -----------------------------------------------------------
def skipped_share(N, L, minf, maxf):
    """band_col_zero in float32: per middle level i = 1 .. L-2, the share of
    the N columns with |sfreq(kx)| > hi_i (a NaN hi, L = 3, compares false)."""
    f = np.float32
    kx = np.arange(N)
    sf = np.where(kx < N // 2, kx, kx - N).astype(f) * (f(1.0) / f(N))
    _, hi = band_edges_f32(L, minf, maxf)
    with np.errstate(invalid="ignore"):
        return [float((np.abs(sf) > hi[i]).mean()) for i in range(1, L - 1)], hi


def test_sfreq_nyquist():
    """sfreq(N/2) = -1/2: the Nyquist column is skipped exactly where hi < 0.5."""
    N = 128
    sh, hi = skipped_share(N, 5, 0.05, 0.45)
    assert [round(100 * s) for s in sh] == [0, 55, 85]        # mm_steer.hpp's figures
    _, hi = band_edges_f32(5, 0.45, 0.50)
    assert all(h >= 0.5 for h in hi.values())


def test_skip_pattern_is_spanned():
    N = 128
    none = most = inverted = seven = False
    for L, minf, maxf, _ in CASES:
        sh, hi = skipped_share(N, L, minf, maxf)
        print(f"L{L}-{minf:g}-{maxf:g}: " + " / ".join(f"{100 * s:.0f} %" for s in sh))
        none |= any(s == 0.0 and hi[i + 1] >= 0.5 for i, s in enumerate(sh))
        most |= any(s >= 0.90 for s in sh)
        # the defaults skip more with every level; an inverted row skips less
        inverted |= any(sh[i + 1] < sh[i] for i in range(len(sh) - 1))
        seven |= L == 7
    assert none and most and inverted and seven, (none, most, inverted, seven)
    assert skipped_share(N, 5, 0.45, 0.50)[0] == [0.0, 0.0, 0.0]
    assert round(100 * max(skipped_share(N, 7, 0.02, 0.60)[0])) == 95     # 121 of 128 columns
    assert [round(100 * s) for s in skipped_share(N, 5, 0.45, 0.10)[0]] == [70, 37, 0]


# ---- 5. the spec's convention on a black frame ---------------------------------------
@pytest.mark.parametrize("filt", [SR.FILTER_DIFF, SR.FILTER_IIR])
def test_spec_black_frame_phase_is_zero(filt):
    """An exactly zero coefficient has phase arctan2(0, 0) = 0 in the spec (no
    -0 reaches arctan2, which would give pi): what test_steer_bands.py's black
    streams hold the kernels to."""
    W, H = 64, 48
    black = np.zeros((H, W, 4))
    black[..., 3] = 1.0
    fr = frames64(W, H, 3)
    r = SR.SteerableRef(W, H, phase_scale=25.0, orientations=8, filt=filt, tau=0.0)
    r.process(fr[0])
    out = r.process(black)
    assert np.all(out[..., :3] == 0) and np.all(out[..., 3] == 1)
    for ph, uh, ul in r.state:
        assert np.all(ph == 0) and not np.signbit(ph).any()
        if filt == SR.FILTER_IIR:
            assert np.isfinite(uh).all() and np.isfinite(ul).all()
    assert np.isfinite(r.process(fr[2])).all()
