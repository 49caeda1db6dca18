#!/usr/bin/env python3
"""What disc covariances (pocs_set_disc_covariances) cost when they are on (DESIGN.md sections 5 and 10).

Legs, one context each, ALTERNATING call by call, the same world in all three -- the bundled room's 7 boxes and tools/discs_probe.py's
8 discs of radius 0.15, 0.80 m beside the plan:
  absent   no covariances: the discs call as it is
  s005     sigma = 0.05 m for every disc at every step
  s020     sigma = 0.20 m growing to 0.60 m over the plan (planio.prediction_covariances, Sd = W; the MC leg persistent)
on
  gmm   bench.py's cfg2 at 20 runs per call: the bundled 56-waypoint plan, K = 3, 10^6 samples per run, samples stored
  mc    bench.py's cfg5 at 64 runs per call in the per-step form: the plan resampled to 500 waypoints, 10^5 particles per run
Timed: the wall time of one pocs_run_gmm_estimation / pocs_run_simulation call.  Median, min and max of the repeats, in ms, and the
ratio to the absent leg.  REACH: per leg the number of (waypoint, uncertain disc) pairs whose grown bounding square lies within
6.67 sigma of the plan's nominal pose with the initial covariance -- a lower bound of what the cull keeps; a call pays a Philox call
and two Box-Muller pairs per pair of poses for those, and nothing for the discs the cull drops.

  python tools/disc_noise_probe.py [--reps 9] [--warm 3] [--only gmm|mc] [--out FILE]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import pocs_amd  # noqa: E402
from discs_probe import discs_beside  # noqa: E402

CASES = ("absent", "s005", "s020")


def covariances(which, W, D):
    if which == "absent":
        return None
    if which == "s005":
        return pocs_amd.planio.prediction_covariances(0.05, 0.0, 1, D)
    return pocs_amd.planio.prediction_covariances(0.20, 0.40 / max(W - 1, 1), W, D)


def reach(plan, fp, discs, cov):
    """(waypoint, uncertain disc) pairs in reach of the nominal pose: |c - p| <= r + footprint radius + 6.67 sigma_disc + 0.5 m."""
    if cov is None:
        return 0
    t = np.asarray(plan["traj"], dtype=np.float64)
    rr = float(np.hypot(fp[2], fp[3]) + np.hypot(fp[0], fp[1]))
    n = 0
    for w in range(len(t)):
        c3 = cov[min(w, len(cov) - 1)]
        for d, (cx, cy, r) in enumerate(discs):
            g = 6.67 * np.sqrt(max(c3[d, 0], c3[d, 2]))
            n += bool(c3[d].any() and abs(cx - t[w, 0]) <= r + rr + g + 0.5 and abs(cy - t[w, 1]) <= r + rr + g + 0.5)
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--only", default=None, choices=["gmm", "mc"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    plan, env = pocs_amd.load_plan(), pocs_amd.load_env()
    long_plan = pocs_amd.resample_plan(plan, 500)
    room = np.asarray(env["boxes"], dtype=np.float64).reshape(-1, 5)
    discs = discs_beside(plan)
    reaches = {}

    def leg(kind, which):
        pl = plan if kind == "gmm" else long_plan
        cov = covariances(which, len(pl["traj"]), len(discs))
        sched = discs if cov is None or len(cov) == 1 else np.repeat(discs[None], len(cov), axis=0)      # (Sd of the discs = Sd of the covariances)
        c = pocs_amd.Context(0)
        c.configure(pl, dict(footprint=env["footprint"], boxes=room, discs=sched, disc_covariances=cov, disc_noise_persistent=True),
                    K=3 if kind == "gmm" else 1, N=1000000 if kind == "gmm" else 100000, seed=0x5EED0001)
        c.set_batch(20 if kind == "gmm" else 64)
        if kind == "mc":
            c.set_option(pocs_amd.OPT_MC_FUSED, 0)
        name = ("gmm cfg2 x20, %s" if kind == "gmm" else "mc cfg5 x64 per-step, %s") % which
        reaches[name] = reach(pl, env["footprint"], discs, cov)
        return name, (c, c.run_gmm_estimation if kind == "gmm" else c.run_simulation)

    legs = [leg(kind, w) for kind in ("gmm", "mc") if args.only in (None, kind) for w in CASES]
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
        base = statistics.median(times[name.rsplit(", ", 1)[0] + ", absent"])
        out.append("%-30s median %8.3f ms   min %8.3f   max %8.3f   x %.4f of absent   (waypoint, uncertain disc) pairs in reach %4d   (p of last call %.6f)" %
                   (name, statistics.median(t), t[0], t[-1], statistics.median(t) / base, reaches[name], probs[name]))
    text = "\n".join(out)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    for _, (c, _) in legs:
        c.close()


if __name__ == "__main__":
    main()
