#!/usr/bin/env python3
"""What prediction hypotheses (pocs_set_disc_hypotheses) cost when they are on (DESIGN.md sections 5 and 10).

Legs, one context each, ALTERNATING call by call, the same world in all of them -- the bundled room's 7 boxes and
tools/discs_probe.py's 8 discs of radius 0.15, 0.80 m beside the plan, each with sigma = 0.05 m (the noise forms' scene):
  noise    covariances alone: the _noise / MC_NOISE forms, the twin the new forms are built on
  hyp      the same, and four of the eight discs gated: two pairs of alternatives {0.6, 0.4} and {0.5, 0.3}: the _hyp / MC_HYP forms
  hyp0     hypotheses without covariances (rows of zeros on the GMM path, MC_HYP without MC_NOISE), against
  discs    the discs alone: the _round / MC_ROUND forms
on
  gmm   bench.py's cfg2 at 20 runs per call: the bundled 56-waypoint plan, K = 3, 10^6 samples per run, samples stored
  mc    bench.py's cfg5 at 64 runs per call in the per-step form: the plan resampled to 500 waypoints, 10^5 particles per run
Timed: the wall time of one pocs_run_gmm_estimation / pocs_run_simulation call.  Median, min and max of the repeats, in ms, the
ratio hyp / noise and hyp0 / discs.  A gated disc in reach costs one Philox-7 call per pair of poses and an integer compare per pose;
a pose for which the disc does not exist takes no part in its narrow phase and forms no Box-Muller pair.

  python tools/disc_hypotheses_probe.py [--reps 9] [--warm 3] [--only gmm|mc] [--out FILE]
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

CASES = ("noise", "hyp", "discs", "hyp0")
GROUP, WEIGHT = (0, 0, -1, 3, 3, -1, -1, -1), (0.6, 0.4, 1.0, 0.5, 0.3, 1.0, 1.0, 1.0)


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

    def leg(kind, which):
        pl = plan if kind == "gmm" else long_plan
        cov = pocs_amd.planio.prediction_covariances(0.05, 0.0, 1, len(discs)) if which in ("noise", "hyp") else None
        hyp = (GROUP, WEIGHT) if which in ("hyp", "hyp0") else None
        c = pocs_amd.Context(0)
        c.configure(pl, dict(footprint=env["footprint"], boxes=room, discs=discs, disc_covariances=cov, disc_noise_persistent=True, disc_hypotheses=hyp),
                    K=3 if kind == "gmm" else 1, N=1000000 if kind == "gmm" else 100000, seed=0x5EED0001)
        c.set_batch(20 if kind == "gmm" else 64)
        if kind == "mc":
            c.set_option(pocs_amd.OPT_MC_FUSED, 0)
        name = ("gmm cfg2 x20, %s" if kind == "gmm" else "mc cfg5 x64 per-step, %s") % which
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
    base_of = dict(noise="noise", hyp="noise", discs="discs", hyp0="discs")
    for name, _ in legs:
        t = sorted(times[name])
        head, which = name.rsplit(", ", 1)
        base = statistics.median(times[head + ", " + base_of[which]])
        out.append("%-30s median %8.3f ms   min %8.3f   max %8.3f   x %.4f of %-5s   (p of last call %.6f)" %
                   (name, statistics.median(t), t[0], t[-1], statistics.median(t) / base, base_of[which], probs[name]))
    text = "\n".join(out)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    for _, (c, _) in legs:
        c.close()


if __name__ == "__main__":
    main()
