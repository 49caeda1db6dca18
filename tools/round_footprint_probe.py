#!/usr/bin/env python3
"""What a round footprint (pocs_set_footprint_disc) costs when it is on (DESIGN.md sections 5 and 10).

The expectation: a call with the disc of radius rho is not slower than the same call with the box footprint {0, 0, rho, rho} on the
same world -- no heading, no axis test.  Legs, one context each, ALTERNATING call by call: two footprints
  box      pocs_set_footprint(0, 0, rho, rho), rho the bundled base's half extent: the bounding square, what a caller had to hand over
  round    pocs_set_footprint_disc(rho)
over three worlds
  room     the bundled room's 7 boxes
  discs    the room and 8 discs of radius 0.15 beside the plan, alternating sides, 0.80 m off its waypoints (tools/discs_probe.py)
  noise    those discs with covariances of sigma = 0.05 m at every step (tools/disc_noise_probe.py's s005; the MC leg persistent)
on
  gmm   bench.py's cfg2 at 20 runs per call: the bundled 56-waypoint plan, K = 3, 10^6 samples per run, samples stored (the
        default), the call as two sub-batches (the default at this size)
  mc    bench.py's cfg5 at 64 runs per call in the per-step form: the plan resampled to 500 waypoints, 10^5 particles per run
Timed: the wall time of one pocs_run_gmm_estimation / pocs_run_simulation call (host chains, upload, graph replay, read-back
included).  Median, min and max of the repeats, in ms, and round against box on the same world.

  python tools/round_footprint_probe.py [--reps 9] [--warm 3] [--only gmm|mc] [--out FILE]
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

sys.path.insert(0, str(Path(__file__).resolve().parent))
from discs_probe import discs_beside  # noqa: E402

WORLDS = ("room", "discs", "noise")
FOOTPRINTS = ("box", "round")


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
    rho = float(env["footprint"][2])
    room = np.asarray(env["boxes"], dtype=np.float64).reshape(-1, 5)

    def leg(kind, world, foot):
        c = pocs_amd.Context(0)
        e = dict(footprint=[0.0, 0.0, rho, rho], boxes=room)
        if foot == "round":
            e["footprint_radius"] = rho
        if world != "room":
            e["discs"] = discs
        if world == "noise":
            e["disc_covariances"] = pocs_amd.planio.prediction_covariances(0.05, 0.0, 1, len(discs))
            e["disc_noise_persistent"] = True
        c.configure(plan if kind == "gmm" else long_plan, e, K=3 if kind == "gmm" else 1, N=1000000 if kind == "gmm" else 100000, seed=0x5EED0001)
        assert (c.footprint_disc() == rho) == (foot == "round")
        c.set_batch(20 if kind == "gmm" else 64)
        if kind == "mc":
            c.set_option(pocs_amd.OPT_MC_FUSED, 0)
        return c, (c.run_gmm_estimation if kind == "gmm" else c.run_simulation)

    legs = []
    for kind, label in (("gmm", "gmm cfg2 x20"), ("mc", "mc cfg5 x64 per-step")):
        if args.only in (None, kind):
            legs += [("%s, %s, %s" % (label, w, f), leg(kind, w, f)) for w in WORLDS for f in FOOTPRINTS]
    times, probs = {name: [] for name, _ in legs}, {}
    for it in range(args.warm + args.reps):
        for name, (c, run) in legs:
            t0 = time.perf_counter()
            p = run()
            dt = time.perf_counter() - t0
            if it >= args.warm:
                times[name].append(dt * 1e3)
            probs[name] = p
    out = ["wall time of one call; %d alternating repeats after %d warm-up calls; rho = %.3f; %s" % (args.reps, args.warm, rho, legs[0][1][0].lib.pocs_version().decode())]
    for name, _ in legs:
        t = sorted(times[name])
        box = statistics.median(times[name.rsplit(", ", 1)[0] + ", box"])
        out.append("%-38s median %8.3f ms   min %8.3f   max %8.3f   x %.4f of box   (p of last call %.6f)" %
                   (name, statistics.median(t), t[0], t[-1], statistics.median(t) / box, probs[name]))
    text = "\n".join(out)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    for _, (c, _) in legs:
        c.close()


if __name__ == "__main__":
    main()
