#!/usr/bin/env python3
"""What round obstacles (pocs_set_discs) cost when they are on (DESIGN.md sections 5 and 10).

Legs, one context each, ALTERNATING call by call, three worlds of the same M + D = 15 records:
  boxes    the bundled room's 7 boxes and 8 boxes out of everything's reach (what every call has run so far)
  discs    the room's 7 boxes and 8 discs of radius 0.15 beside the plan, alternating sides, 0.80 m off its waypoints
  squares  the room's 7 boxes and those discs' bounding squares as boxes (what a caller had to hand over before)
on
  gmm   bench.py's cfg2 at 20 runs per call: the bundled 56-waypoint plan, K = 3, 10^6 samples per run, samples stored (the
        default), the call as two sub-batches (the default at this size)
  mc    bench.py's cfg5 at 64 runs per call in the per-step form: the plan resampled to 500 waypoints, 10^5 particles per run
Timed: the wall time of one pocs_run_gmm_estimation / pocs_run_simulation call (host chains, upload, graph replay, read-back
included).  Median, min and max of the repeats, in ms, the ratio to the boxes leg, and discs against squares.

  python tools/discs_probe.py [--reps 9] [--warm 3] [--only gmm|mc] [--out FILE]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import pocs_amd  # noqa: E402

WORLDS = ("boxes", "discs", "squares")


def discs_beside(plan, n=8, off=0.80, r=0.15):
    """n discs beside the plan: at n waypoints spread over it, `off` to the left and right of the heading in turn."""
    t = np.asarray(plan["traj"], dtype=np.float64)
    idx = np.linspace(2, len(t) - 3, n).astype(int)
    out = []
    for j, i in enumerate(idx):
        side = 1.0 if j % 2 == 0 else -1.0
        out.append([t[i, 0] - side * off * np.sin(t[i, 2]), t[i, 1] + side * off * np.cos(t[i, 2]), r])
    return np.array(out)


def world_of(env, discs, which):
    """(boxes, discs) of a leg: 15 records each."""
    room = np.asarray(env["boxes"], dtype=np.float64).reshape(-1, 5)
    if which == "boxes":
        far = np.array([[60.0 + 2.0 * j, 40.0, 0.15, 0.15, 0.0] for j in range(len(discs))])
        return np.vstack([room, far]), None
    if which == "squares":
        return np.vstack([room, np.column_stack([discs[:, 0], discs[:, 1], discs[:, 2], discs[:, 2], np.zeros(len(discs))])]), None
    return room, discs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--only", default=None, choices=["gmm", "mc"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    plan, env = pocs_amd.load_plan(), pocs_amd.load_env()
    long_plan = pocs_amd.resample_plan(plan, 500)
    discs = discs_beside(plan)

    def gmm(which):
        boxes, d = world_of(env, discs, which)
        c = pocs_amd.Context(0)
        c.configure(plan, dict(footprint=env["footprint"], boxes=boxes, discs=d), K=3, N=1000000, seed=0x5EED0001)
        c.set_batch(20)
        return c, c.run_gmm_estimation

    def mc(which):
        boxes, d = world_of(env, discs, which)
        c = pocs_amd.Context(0)
        c.configure(long_plan, dict(footprint=env["footprint"], boxes=boxes, discs=d), K=1, N=100000, seed=0x5EED0001)
        c.set_batch(64)
        c.set_option(pocs_amd.OPT_MC_FUSED, 0)
        return c, c.run_simulation

    legs = []
    if args.only in (None, "gmm"):
        legs += [("gmm cfg2 x20, %s" % w, gmm(w)) for w in WORLDS]
    if args.only in (None, "mc"):
        legs += [("mc cfg5 x64 per-step, %s" % w, mc(w)) for w in WORLDS]
    times, probs = {name: [] for name, _ in legs}, {}
    for it in range(args.warm + args.reps):
        for name, (c, run) in legs:
            t0 = time.perf_counter()
            p = run()
            dt = time.perf_counter() - t0
            if it >= args.warm:
                times[name].append(dt * 1e3)
            probs[name] = p
    out = ["wall time of one call; %d alternating repeats after %d warm-up calls; %s" % (args.reps, args.warm, legs[0][1][0].lib.pocs_version().decode())]
    for name, _ in legs:
        t = sorted(times[name])
        head = name.rsplit(", ", 1)[0]
        base, sq = statistics.median(times[head + ", boxes"]), statistics.median(times[head + ", squares"])
        out.append("%-34s median %8.3f ms   min %8.3f   max %8.3f   x %.4f of boxes   x %.4f of squares   (p of last call %.6f)" %
                   (name, statistics.median(t), t[0], t[-1], statistics.median(t) / base, statistics.median(t) / sq, probs[name]))
    text = "\n".join(out)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    for _, (c, _) in legs:
        c.close()


if __name__ == "__main__":
    main()
