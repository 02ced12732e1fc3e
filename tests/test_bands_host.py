"""K2's band layouts over the frequency sliders, host side (no GPU).

The spectral operation of K2 is chosen from (levels, min_freq, max_freq):
mm_create / mm_set_params classify the middle bands (csrc/mm_impl.hpp,
build_spec -> bands_fit_table, bands_overlap) into

  TAB      no two middle bands overlap        MM_K2_PYR_TAB, one-band op
  TAB2     two overlap, no three do           MM_K2_PYR_TAB2, per-wave one-/two-band op
  GENERIC  three share an interval            MM_MODE_PYRAMID, masks per bin and frame

CASES is the table of slider points that tests/test_bands.py runs on the
GPU.  This file keeps the table honest: a float32 restatement of the host
classifier puts every row in its stated class, the oracle is pinned against
the float64 twin at every row (so a GPU failure there is about the kernels),
and the twin's masks show that every TAB2 row has both one-band and two-band
columns at the sizes the GPU tests use.
"""
import numpy as np
import pytest

import np_twin
import oracle_py as O

TAB, TAB2, GENERIC = "TAB", "TAB2", "GENERIC"

# (levels, min_freq, max_freq, class).  The reference's Inspector ranges are
# minFrequency [0.05, 0.45], maxFrequency [0.1, 0.5]; 0.02 / 0.6 and the
# inverted rows lie outside them and are legal through the ABI
# (validate_params asks only for > 0).
CASES = [
    (5, 0.05, 0.45, TAB),        # the defaults: anchors
    (6, 0.05, 0.45, TAB2),
    (4, 0.05, 0.50, TAB),
    (5, 0.05, 0.50, TAB),
    (4, 0.45, 0.10, TAB),        # inverted
    (6, 0.02, 0.60, TAB),        # gaps between bands
    (4, 0.20, 0.45, TAB2),
    (4, 0.05, 0.10, TAB2),
    (5, 0.05, 0.30, TAB2),
    (5, 0.15, 0.50, TAB2),
    (5, 0.45, 0.10, TAB2),       # inverted
    (6, 0.05, 0.30, TAB2),
    (7, 0.05, 0.50, TAB2),
    (7, 0.02, 0.60, TAB2),
    (5, 0.10, 0.20, GENERIC),
    # (not (5, 0.10, 0.30): its three bands meet in one point, [0.15, 0.15],
    # which float64 opens by an ulp and the host's float32 closes: TAB2 there)
    (5, 0.10, 0.25, GENERIC),
    (5, 0.45, 0.50, GENERIC),
    (5, 0.25, 0.25, GENERIC),    # all bands coincide
    (6, 0.10, 0.20, GENERIC),
    (6, 0.20, 0.45, GENERIC),
    (2, 0.30, 0.35, TAB),        # no middle band
    (3, 0.10, 0.30, TAB),        # the NaN band (0 / 0 ratio): compares false everywhere
]


def case_id(c):
    return f"L{c[0]}-{c[1]:g}-{c[2]:g}"


def rows_of(cls):
    return [c for c in CASES if c[3] == cls]


# ---- 1. the host classifier, restated in float32 ------------------------------
def band_edges_f32(L, minf, maxf):
    """build_spec's lo / hi of the middle bands, np.float32 in its order."""
    f = np.float32
    minf, maxf = f(minf), f(maxf)
    lo, hi = {}, {}
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(1, L - 1):
            ratio = f(i - 1) / f(L - 3)
            center = minf * np.power(maxf / minf, f(1.0) - ratio, dtype=f)
            bwid = center * f(0.5)
            lo[i], hi[i] = f(center - bwid), f(center + bwid)
    return lo, hi


def classify_f32(L, minf, maxf):
    """bands_fit_table and bands_overlap (the 1e-5 * hi rule included)."""
    lo, hi = band_edges_f32(L, minf, maxf)
    mid = range(1, L - 1)
    fit = True
    for a in mid:
        for b in range(a + 1, L - 1):
            for c in range(b + 1, L - 1):
                if np.fmax(lo[a], np.fmax(lo[b], lo[c])) < np.fmin(hi[a], np.fmin(hi[b], hi[c])):
                    fit = False
    overlap = False
    for a in mid:
        for b in range(a + 1, L - 1):
            l2, h2 = np.fmax(lo[a], lo[b]), np.fmin(hi[a], hi[b])
            if h2 - l2 > np.float32(1e-5) * h2:
                overlap = True
    if not fit:
        return GENERIC
    return TAB2 if overlap else TAB


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_classifier_mirror(case):
    L, minf, maxf, cls = case
    assert classify_f32(L, minf, maxf) == cls


def test_table_spans_classes_and_levels():
    assert len(CASES) == len(set(CASES)) == 22
    for cls in (TAB, TAB2, GENERIC):
        assert len({c[0] for c in rows_of(cls) if c[0] >= 4}) >= 2, cls
    # the defaults stay in as anchors
    assert (5, 0.05, 0.45, TAB) in CASES and (6, 0.05, 0.45, TAB2) in CASES


# ---- 2. the oracle pinned over the square ------------------------------------
def _pair(W, H):
    return [O.synth_frame(W, H, t).astype(np.float32) / 255 for t in (0, 3)]


def _oracle_vs_twin(L, minf, maxf, S, edge, tau=0.01):
    W, H = 64, 48
    f0, f1 = _pair(W, H)
    o = O.Oracle(W, H, levels=L, min_freq=minf, max_freq=maxf, phase_scale=S, mag_threshold=tau,
                 edge_mode=edge)
    o.process(f0)
    a = o.process(f1)
    o.close()
    b = np_twin.process_frame(f1.astype(np.float64), f0.astype(np.float64), L, minf, maxf, S,
                              tau=tau, edge=edge)
    e = np.abs(a - b)
    mx, rmse = e.max(), np.sqrt((e ** 2).mean())
    print(f"oracle vs twin: max {mx:.3g} rmse {rmse:.3g}")
    assert mx < 5e-6 and rmse < 1e-6, (mx, rmse)


@pytest.mark.parametrize("k", range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_oracle_vs_twin_over_square(k):
    L, minf, maxf, _ = CASES[k]
    _oracle_vs_twin(L, minf, maxf, 25.0, k & 1)


@pytest.mark.parametrize("tau", [0.0, 0.001])
@pytest.mark.parametrize("case", [(5, 0.05, 0.50, TAB), (5, 0.05, 0.30, TAB2), (6, 0.10, 0.20, GENERIC)],
                         ids=case_id)
def test_oracle_vs_twin_threshold(case, tau):
    """tau = 0 (nothing gated) and a small tau: one gate decision that differs
    between fp32 and float64 moves a pixel by at most 2 tau / N^2 = 5e-7."""
    L, minf, maxf, _ = case
    _oracle_vs_twin(L, minf, maxf, 25.0, 0, tau=tau)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_oracle_masks_vs_twin(case):
    L, minf, maxf, _ = case
    n = 256
    tw = np_twin.masks(n, L, minf, maxf)
    for i in range(L):
        assert np.abs(O.mask(n, L, i, minf, maxf) - tw[i]).max() < 1e-5, i


# ---- 3. which bins hold how many middle bands --------------------------------
# A mask counts as present above EPS: bands that only touch (TAB layouts) meet
# where both raised cosines are 0 up to rounding (~1e-30 in float64).
EPS = 1e-9


def middle_count(N, L, minf, maxf):
    """[fx = 0 .. N/2][fy = 0 .. N): number of middle masks present at the bin
    (K2's columns: the half spectrum, unshifted)."""
    m = np_twin.masks(N, L, minf, maxf)
    cnt = np.zeros((N, N), np.int64)
    for i in range(1, L - 1):
        cnt += m[i] > EPS
    cnt = np.fft.ifftshift(cnt)            # [fy][fx], DC at (0, 0)
    return cnt[:, :N // 2 + 1].T


@pytest.mark.parametrize("N", [64, 256])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_band_count_per_bin(case, N):
    """The twin's masks agree with the class; TAB2 rows have columns of both
    kinds, so the GPU cases run both wave branches of MM_K2_PYR_TAB2."""
    L, minf, maxf, cls = case
    cnt = middle_count(N, L, minf, maxf)
    per_col = cnt.max(axis=1)
    if cls == TAB:
        assert cnt.max() <= 1
    elif cls == TAB2:
        assert cnt.max() == 2
        assert (per_col <= 1).any(), "no column of one-band bins only"
        assert (per_col == 2).any(), "no column with a two-band bin"
        assert (cnt == 0).any() and (cnt == 1).any()
    elif N == 256:
        assert cnt.max() >= 3
