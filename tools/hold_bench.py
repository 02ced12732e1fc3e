#!/usr/bin/env python3
"""A held reference frame (mm_set_hold) against the rolling stream and against
the workaround it replaces.

Workload: 1920x1080 RGBA8, L = 5, S = 25, the bench's 300-frame stream in
mm_process_stream calls of the default batch.  Legs, `--runs` runs each (wall
clock between two device synchronisations, after one untimed pass), then one
more pass under mm_profile_* for the device time per kernel and frame:

  a  the rolling stream (hold off)
  b  the hold stream: mm_set_hold(1), every frame against the first one
  c  the workaround: one mm_set_state(R) plus one mm_process per frame
  d  16 lanes, one mm_process_lanes per tick: all rolling, then all held

A leg's spread is the distance between its runs.  With MM355_LIB naming a
library from before the hold, legs b and the held half of d are left out (the
parent's figures for a, c and d beside the new library's).  One JSON document on
stdout, and in --out.

usage: python tools/hold_bench.py [--frames 300] [--runs 2] [--lanes 16] [--ticks 100]
                                  [--out profiles/hold_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "phase-based-motion-manipulation_amd"))

import torch  # noqa: E402
import mm355  # noqa: E402

RING = 4   # ticks of input frames held per lane


def params():
    return mm355.Params.make(levels=5, phase_scale=25.0)


def kernel_us(prof):
    """mm_profile_end -> K1 / K2 / K34 device microseconds per frame."""
    name = {"k_rows_fwd": "K1", "k_cols": "K2", "k_rows_inv_compose": "K34", "k_rows_inv": "K3", "k_compose": "K4"}
    return {name[k]: round(1e3 * ms / f, 3) for k, (ms, n, f) in prof.items() if f}


def leg(setup, step, frames, runs):
    """frames/s of `runs` timed passes, after one untimed pass."""
    setup()
    step()
    torch.cuda.synchronize()
    fps = []
    for _ in range(runs):
        setup()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        fps.append(frames / (time.perf_counter() - t0))
    return fps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--lanes", type=int, default=16)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H, n, fmt = a.width, a.height, a.frames, mm355.RGBA8
    hold = mm355.has_hold()
    doc = {"width": W, "height": H, "levels": 5, "phase_scale": 25.0, "frames": n, "runs": a.runs,
           "library": os.path.relpath(mm355.binding.library_path(), ROOT), "has_hold": hold, "legs": {}}
    h = mm355.Handle(W, H, params())
    doc["batch"] = h.batch
    src = torch.empty((n, H, W, 4), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    h.synth(src, 0, n)
    R = torch.zeros(h.state_bytes, dtype=torch.uint8, device="cuda")
    h.compute_state(src[0], fmt, R)
    torch.cuda.synchronize()

    def record(name, fps, prof, per=None):
        row = {"fps": [round(v, 1) for v in fps], "fps_mean": round(sum(fps) / len(fps), 1),
               "spread_fps": round(max(fps) - min(fps), 1), "kernel_us_per_frame": kernel_us(prof)}
        if per:
            row.update(per)
        doc["legs"][name] = row
        print(name, json.dumps(row), file=sys.stderr, flush=True)

    def profiled(setup, step):
        setup()
        h.profile_begin()
        step()
        torch.cuda.synchronize()
        return h.profile_end()

    def stream():
        h.process_stream(src, dst, n, fmt)

    def per_frame():
        for k in range(n):
            h.set_state(R)
            h.process(src[k], dst[k], fmt)

    def rolling():
        if hold:
            h.set_hold(False)
        h.set_state(R)

    def held():
        h.set_hold(True)
        h.set_state(R)

    record("a_rolling_stream", leg(rolling, stream, n, a.runs), profiled(rolling, stream))
    if hold:
        record("b_hold_stream", leg(held, stream, n, a.runs), profiled(held, stream))
    record("c_set_state_per_frame", leg(rolling, per_frame, n, a.runs), profiled(rolling, per_frame))
    if hold:
        h.set_hold(False)
    # d: lanes, one frame of each per tick
    M = a.lanes
    lay = mm355.Surface.tight(W, H, fmt)
    h.set_batch(1)
    h.set_lanes(M)
    lsrc = src[:RING * M].reshape(RING, M, H, W, 4)
    ldst = dst[:M]

    def ticks():
        for t in range(a.ticks):
            h.process_lanes(lsrc[t % RING], lay, ldst, lay)

    def lanes_rolling():
        if hold:
            h.set_lanes_hold(0)
        h.reset_lane()
        h.process_lanes(lsrc[0], lay, ldst, lay)      # every lane has state before the timed ticks

    def lanes_held():
        h.set_lanes_hold((1 << M) - 1)
        h.reset_lane()
        h.process_lanes(lsrc[0], lay, ldst, lay)

    per = {"lanes": M, "ticks": a.ticks}
    record("d_lanes_rolling", leg(lanes_rolling, ticks, M * a.ticks, a.runs), profiled(lanes_rolling, ticks), per)
    if hold:
        record("d_lanes_held", leg(lanes_held, ticks, M * a.ticks, a.runs), profiled(lanes_held, ticks), per)
        L = doc["legs"]
        doc["b_over_c"] = round(L["b_hold_stream"]["fps_mean"] / L["c_set_state_per_frame"]["fps_mean"], 2)
        doc["b_over_a"] = round(L["b_hold_stream"]["fps_mean"] / L["a_rolling_stream"]["fps_mean"], 3)
        doc["d_held_over_rolling"] = round(L["d_lanes_held"]["fps_mean"] / L["d_lanes_rolling"]["fps_mean"], 3)
    h.close()
    txt = json.dumps(doc, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
