#!/usr/bin/env python3
"""Existing paths of two libmm355.so builds against each other in one session.

The two libraries alternate, `--runs` runs each (`--order parent`: parent 1,
new 1, parent 2, new 2; `--order new`: the new library first), every step a
process of its own with MM355_LIB naming the parent's library or unset:

  bench.py --gpus 1 --steps 3 --warmup 2 --no-cpu-baseline      frames/s
  tools/fmt_bench.py (tight legs, no convert or BGRA legs: the  median frames/s of RGBA8, NV12, P010
                      same legs in every round for both)
  tools/lanes_bench.py --lanes 8,16,64 --no-formats             leg c (mm_process_lanes): the mean of a run's
                                                                passes, and K2's device time per lane-frame

A figure "holds" when every run of the new library lies within the parent's
own run-to-run range; the others are listed with both sets of numbers.  One
JSON document on stdout, and in --out.  A step that fails or runs past its
time limit ends the whole run.

usage: python tools/ab_gate.py --parent PATH/libmm355.so [--order parent|new] [--runs 2] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def step(args, lib, limit):
    env = {k: v for k, v in os.environ.items() if k != "MM355_LIB"}
    if lib:
        env["MM355_LIB"] = lib
    r = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=limit)
    if r.returncode:
        sys.exit(f"{' '.join(args)}: exit {r.returncode}\n{r.stderr[-2000:]}")
    return r.stdout


def one_run(lib, tmp):
    out = {}
    txt = step(["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2", "--no-cpu-baseline"], lib, 150)
    out["bench_py"] = next(json.loads(l)["value"] for l in reversed(txt.splitlines()) if l.lstrip().startswith("{"))
    f = os.path.join(tmp, "fmt.json")
    step(["tools/fmt_bench.py", "--rounds", "3", "--leg-seconds", "0.3", "--no-pitched", "--no-convert", "--no-bgra", "--out", f], lib, 240)
    fm = json.load(open(f))["formats"]
    for name in ("rgba8", "nv12", "p010"):
        out["fmt_bench_" + name] = fm[name]["fps_median"]
    f = os.path.join(tmp, "lanes.json")
    step(["tools/lanes_bench.py", "--lanes", "8,16,64", "--no-formats", "--out", f], lib, 240)
    for row in json.load(open(f))["rows"]:
        out[f"lanes_bench_c_M{row['lanes']}"] = round(sum(row["c_fps"]) / len(row["c_fps"]), 1)
        out[f"k_cols_us_per_lane_frame_M{row['lanes']}"] = row["c_kernel_us_per_lane_frame"].get("k_cols")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="the parent build's libmm355.so")
    ap.add_argument("--order", choices=("parent", "new"), default="parent", help="which library runs first in each pair")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    parent = os.path.abspath(a.parent)
    order = ("parent", "new") if a.order == "parent" else ("new", "parent")
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for run in range(a.runs):
            for which in order:
                r = one_run(parent if which == "parent" else None, tmp)
                print(which, run + 1, json.dumps(r), file=sys.stderr, flush=True)
                for k, v in r.items():
                    res.setdefault(k, {"parent": [], "new": []})[which].append(v)
    for k, v in res.items():
        if k.startswith("k_cols"):
            continue    # (a time: reported, not gated)
        lo, hi = min(v["parent"]), max(v["parent"])
        v["parent_spread"] = round(hi - lo, 1)
        v["holds"] = all(lo <= x <= hi for x in v["new"])
        v["new_outside_by"] = [round(x - hi if x > hi else x - lo if x < lo else 0.0, 1) for x in v["new"]]
    doc = {"order": list(order), "runs": a.runs, "figures": res}
    txt = json.dumps(doc, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
