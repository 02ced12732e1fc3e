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

RGBA8 at every M of --lanes, and NV12 and Y8 at M = 16.  A leg's spread is the
distance between its runs.  "holds": leg c exceeds leg a by more than the larger
of the two legs' spreads.  One JSON document on stdout, and in --out.

usage: python tools/lanes_bench.py [--lanes 1,2,4,8,16,32,64] [--ticks 200] [--warmup 20]
                                   [--runs 2] [--out profiles/lanes_bench.json]
"""
import argparse
import json
import os
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--lanes", default="1,2,4,8,16,32,64")
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H = a.width, a.height
    out = {"width": W, "height": H, "levels": 5, "phase_scale": 25.0, "ticks": a.ticks, "warmup": a.warmup,
           "runs": a.runs, "library": os.path.relpath(mm355.binding.library_path(), ROOT), "rows": []}
    for M in [int(v) for v in a.lanes.split(",")]:
        out["rows"].append(bench(W, H, M, mm355.RGBA8, "rgba8", a))
        print(json.dumps(out["rows"][-1]), file=sys.stderr, flush=True)
    for fmt, name in ((mm355.NV12, "nv12"), (mm355.Y8, "y8")):
        out["rows"].append(bench(W, H, 16, fmt, name, a))
        print(json.dumps(out["rows"][-1]), file=sys.stderr, flush=True)
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
