#!/usr/bin/env python3
"""One frame of M live streams per tick: M one-frame calls against one
mm_process_lanes call.

M synthetic streams of one geometry (default 1920x1080, L = 5, S = 25) deliver
one frame each per tick.  Three legs per M, `--warmup` ticks and then `--ticks`
timed ticks (wall clock between two device synchronisations), `--runs` runs each:

  a  M handles, one mm_process each per tick, all on one stream
  b  the same, each handle on its own stream (mm_stream)
  c  one handle with M lanes, one mm_process_lanes per tick; then one more
     pass under mm_profile_* for the device time per kernel

RGBA8 at every M of --lanes, and NV12 and Y8 at M = 16 (--no-formats: RGBA8
only).  A leg's spread is the distance between its runs.  "holds": leg c
exceeds leg a by more than the larger of the two legs' spreads.  One JSON
document on stdout, and in --out.

--mask adds, per M, the legs of mm_process_lanes_mask (sources that are not
genlocked): frames/s there are over the frames actually processed.

  full    the mask of all lanes, against leg c of the same library
  rates   two rate groups, lanes ordered by group: the upper half of the lanes
          takes a frame every second tick; against rates_2h, today's way: two
          handles of M/2 lanes, one mm_process_lanes each at its own rate
  drops   every (lane, tick) slot dropped with probability 0.05 (seeded);
          against `full`, and against drops_1f, today's way for such a rig: M
          handles and a one-frame call per frame that arrived (leg a's pattern)

with the device time per kernel and lane-frame (mm_profile_*) and the launches
per tick of each kernel, which for the forward row kernel is the number of runs
the masks and the lanes' bank bits break a tick into.

usage: python tools/lanes_bench.py [--lanes 1,2,4,8,16,32,64] [--ticks 200] [--warmup 20]
                                   [--runs 2] [--no-formats] [--mask] [--out profiles/lanes_bench.json]
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "phase-based-motion-manipulation_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import mm355  # noqa: E402
from fmt_bench import to_420, to_mono  # noqa: E402

RING = 4   # ticks of input frames held per lane


def make_inputs(W, H, M, fmt):
    """[RING][M] frames of `fmt` on the device: lane k is a synthetic stream of its own."""
    h = mm355.Handle(W, H, mm355.Params.make())
    tmp = torch.empty((RING, H, W, 4), dtype=torch.uint8, device="cuda")
    src = None
    for k in range(M):
        h.synth(tmp, 3 * k, RING, seed=0x5EED0000 + 977 * k)
        torch.cuda.synchronize()
        f = tmp if fmt == mm355.RGBA8 else to_420(torch, tmp) if fmt == mm355.NV12 else to_mono(torch, tmp, 8)
        if src is None:
            src = torch.empty((RING, M) + tuple(f.shape[1:]), dtype=f.dtype, device="cuda")
        src[:, k] = f
    torch.cuda.synchronize()
    h.close()
    return src


def timed(step, ticks, warmup):
    for t in range(warmup):
        step(t)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(ticks):
        step(t)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def bench(W, H, M, fmt, name, a):
    params = lambda: mm355.Params.make(levels=5, phase_scale=25.0)
    src = make_inputs(W, H, M, fmt)
    dst = torch.empty_like(src[0])
    lay = mm355.Surface.tight(W, H, fmt)
    row = {"format": name, "lanes": M}
    # a, b: today's way, a handle per stream (one-frame batches: two G slots and a Q slot each)
    hs = []
    for _ in range(M):
        h = mm355.Handle(W, H, params())
        h.set_batch(1)
        hs.append(h)

    def one_stream(t):
        for k, h in enumerate(hs):
            h.process(src[t % RING, k], dst[k], fmt)

    def own_streams(t):
        for k, h in enumerate(hs):
            h.process(src[t % RING, k], dst[k], fmt, stream=h.stream)

    for leg, step in (("a", one_stream), ("b", own_streams)):
        row[leg + "_fps"] = [M * a.ticks / timed(step, a.ticks, a.warmup) for _ in range(a.runs)]
    for h in hs:
        h.close()
    # c: one call per tick
    hl = mm355.Handle(W, H, params())
    hl.set_batch(1)
    hl.set_lanes(M)

    def lanes(t):
        hl.process_lanes(src[t % RING], lay, dst, lay)

    row["c_fps"] = [M * a.ticks / timed(lanes, a.ticks, a.warmup) for _ in range(a.runs)]
    hl.profile_begin()
    for t in range(a.ticks):
        lanes(t)
    torch.cuda.synchronize()
    prof = hl.profile_end()
    row["c_kernel_us_per_lane_frame"] = {k: round(1e3 * ms / f, 3) for k, (ms, n, f) in prof.items() if f}
    row["c_kernel_us_per_tick"] = {k: round(1e3 * ms / n, 3) for k, (ms, n, f) in prof.items() if n}
    hl.close()
    mean = lambda v: sum(v) / len(v)
    spread = lambda v: max(v) - min(v)
    row["c_over_a"] = round(mean(row["c_fps"]) / mean(row["a_fps"]), 3)
    row["c_over_b"] = round(mean(row["c_fps"]) / mean(row["b_fps"]), 3)
    row["spread_fps"] = {leg: round(spread(row[leg + "_fps"]), 1) for leg in "abc"}
    row["holds"] = mean(row["c_fps"]) - mean(row["a_fps"]) > max(spread(row["a_fps"]), spread(row["c_fps"]))
    for leg in "abc":
        row[leg + "_fps"] = [round(v, 1) for v in row[leg + "_fps"]]
    return row


def bench_mask(W, H, M, a):
    """The mask legs at RGBA8 (the module's docstring)."""
    fmt = mm355.RGBA8
    params = lambda: mm355.Params.make(levels=5, phase_scale=25.0)
    src = make_inputs(W, H, M, fmt)
    dst = torch.empty_like(src[0])
    lay = mm355.Surface.tight(W, H, fmt)
    full, low = (1 << M) - 1, (1 << (M // 2)) - 1
    total = a.warmup + a.ticks
    rng = random.Random(0x5EED0000 + M)
    sched = {"full": [full] * total,
             "rates": [full if t % 2 == 0 else low for t in range(total)],
             "drops": [sum(1 << k for k in range(M) if rng.random() >= 0.05) for _ in range(total)]}
    row = {"format": "rgba8", "lanes": M, "drop_probability": 0.05}

    def run(step, masks):
        """frames/s over the frames of the timed ticks (step(t, mask), t counted from the first warm-up tick)"""
        out = []
        frames = sum(bin(m).count("1") for m in masks[a.warmup:])
        for _ in range(a.runs):
            for t in range(a.warmup):
                step(t, masks[t])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(a.warmup, total):
                step(t, masks[t])
            torch.cuda.synchronize()
            out.append(frames / (time.perf_counter() - t0))
        return out

    hl = mm355.Handle(W, H, params())
    hl.set_batch(1)
    hl.set_lanes(M)
    row["c_fps"] = run(lambda t, m: hl.process_lanes(src[t % RING], lay, dst, lay), sched["full"])
    for leg, masks in sched.items():
        hl.reset_lane()
        row[leg + "_fps"] = run(lambda t, m: hl.process_lanes_mask(m, src[t % RING], lay, dst, lay), masks)
        hl.profile_begin()
        for t in range(a.warmup, total):
            hl.process_lanes_mask(masks[t], src[t % RING], lay, dst, lay)
        torch.cuda.synchronize()
        prof = hl.profile_end()
        row[leg + "_kernel_us_per_lane_frame"] = {k: round(1e3 * ms / f, 3) for k, (ms, n, f) in prof.items() if f}
        row[leg + "_launches_per_tick"] = {k: round(n / a.ticks, 2) for k, (ms, n, f) in prof.items() if n}
        row[leg + "_lane_frames_per_tick"] = round(sum(bin(m).count("1") for m in masks[a.warmup:]) / a.ticks, 2)
    hl.close()
    # rates_2h: a handle per rate group
    hh = []
    for _ in range(2):
        h = mm355.Handle(W, H, params())
        h.set_batch(1)
        h.set_lanes(M // 2)
        hh.append(h)

    def two_handles(t, m):
        hh[0].process_lanes(src[t % RING, :M // 2], lay, dst[:M // 2], lay)
        if m == full:
            hh[1].process_lanes(src[t % RING, M // 2:], lay, dst[M // 2:], lay)

    row["rates_2h_fps"] = run(two_handles, sched["rates"])
    for h in hh:
        h.close()
    # drops_1f: a handle per stream, a call per frame that arrived
    hs = []
    for _ in range(M):
        h = mm355.Handle(W, H, params())
        h.set_batch(1)
        hs.append(h)

    def one_frame_calls(t, m):
        for k, h in enumerate(hs):
            if (m >> k) & 1:
                h.process(src[t % RING, k], dst[k], fmt)

    row["drops_1f_fps"] = run(one_frame_calls, sched["drops"])
    for h in hs:
        h.close()
    mean = lambda v: sum(v) / len(v)
    legs = ("c", "full", "rates", "rates_2h", "drops", "drops_1f")
    row["full_over_c"] = round(mean(row["full_fps"]) / mean(row["c_fps"]), 3)
    row["rates_over_2h"] = round(mean(row["rates_fps"]) / mean(row["rates_2h_fps"]), 3)
    row["drops_over_full"] = round(mean(row["drops_fps"]) / mean(row["full_fps"]), 3)
    row["drops_over_1f"] = round(mean(row["drops_fps"]) / mean(row["drops_1f_fps"]), 3)
    row["spread_fps"] = {leg: round(max(row[leg + "_fps"]) - min(row[leg + "_fps"]), 1) for leg in legs}
    for leg in legs:
        row[leg + "_fps"] = [round(v, 1) for v in row[leg + "_fps"]]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--lanes", default="1,2,4,8,16,32,64")
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--no-formats", action="store_true", help="leave the NV12 and Y8 rows out")
    ap.add_argument("--mask", action="store_true", help="the mm_process_lanes_mask legs instead (even lane counts)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H = a.width, a.height
    out = {"width": W, "height": H, "levels": 5, "phase_scale": 25.0, "ticks": a.ticks, "warmup": a.warmup,
           "runs": a.runs, "library": os.path.relpath(mm355.binding.library_path(), ROOT), "rows": []}
    for M in [int(v) for v in a.lanes.split(",")]:
        out["rows"].append(bench_mask(W, H, M, a) if a.mask else bench(W, H, M, mm355.RGBA8, "rgba8", a))
        print(json.dumps(out["rows"][-1]), file=sys.stderr, flush=True)
    for fmt, name in () if a.mask or a.no_formats else ((mm355.NV12, "nv12"), (mm355.Y8, "y8")):
        out["rows"].append(bench(W, H, 16, fmt, name, a))
        print(json.dumps(out["rows"][-1]), file=sys.stderr, flush=True)
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
