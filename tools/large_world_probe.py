#!/usr/bin/env python3
"""What a large collision world costs (pocs_set_world with more than 64 boxes; DESIGN.md sections 5 and 10;
profiles/large_world_probe.txt).

Legs, one context each, ALTERNATING call by call: the bundled room (7 boxes) through set_env -- the small-world path, the kernels
of the parent commit -- against the room plus far-away clutter to 65, 1024 and 4096 boxes through set_world.  The clutter lies at
x in [20, 60], out of every pose's reach, so every leg computes the same probability: what differs is the cull.
  gmm   bench.py's cfg2 at 20 runs per call: the bundled 56-waypoint plan, K = 3, 10^6 samples per run, samples stored (the
        default), the call as two sub-batches (the default at this size); under a large world one k_world_cull launch in front of
        every sampling launch
  mc    bench.py's cfg5 at 64 runs per call: the plan resampled to 500 waypoints, 10^5 particles per run, the per-step launch
        form (the fused form is refused under a large world)
Timed: the wall time of one pocs_run_gmm_estimation / pocs_run_simulation call (host chains, upload, graph replay, read-back).
Median, min and max of the repeats, in ms.  The share of k_world_cull in a call's kernel time is not measured here: run ONE leg
under a kernel trace (--only gmm --boxes 4096 --reps 1 --warm 1) and read the trace's statistics.

  python tools/large_world_probe.py [--reps 12] [--warm 3] [--only gmm|mc] [--boxes 7,65,1024,4096] [--out FILE]
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


def clutter(env, M, seed=11):
    """The room's boxes plus M - 7 random boxes far away, the table shuffled (as tests/test_large_world.py builds it)."""
    room = np.asarray(env["boxes"], np.float64).reshape(-1, 5)
    rng = np.random.default_rng(seed)
    n = M - len(room)
    far = np.column_stack([rng.uniform(20.0, 60.0, n), rng.uniform(-2.0, 2.0, n), rng.uniform(0.05, 0.4, n), rng.uniform(0.05, 0.4, n),
                           np.where(rng.random(n) < 0.3, 0.0, rng.uniform(-3.2, 3.2, n))])
    return rng.permutation(np.vstack([room, far]), axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--only", default=None, choices=["gmm", "mc"])
    ap.add_argument("--boxes", default="7,65,1024,4096", help="worlds to time: 7 = the room through set_env, more = clutter through set_world")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = [int(t) for t in args.boxes.split(",")]
    plan, env = pocs_amd.load_plan(), pocs_amd.load_env()
    long_plan = pocs_amd.resample_plan(plan, 500)

    def world(c, M):
        if M > 7:
            c.set_world(clutter(env, M))
        assert c.world_boxes() == M

    def gmm(M):
        c = pocs_amd.Context(0)
        c.configure(plan, env, K=3, N=1000000, seed=0x5EED0001)
        c.set_batch(20)
        world(c, M)
        return c, c.run_gmm_estimation

    def mc(M):
        c = pocs_amd.Context(0)
        c.configure(long_plan, env, K=1, N=100000, seed=0x5EED0001)
        c.set_batch(64)
        world(c, M)
        return c, c.run_simulation

    legs = []
    for kind, make in (("gmm cfg2 x20", gmm), ("mc cfg5 x64 per-step", mc)):
        if args.only in (None, kind[:3].strip()):
            legs += [("%s, %4d boxes (%s)" % (kind, M, "set_env" if M <= 7 else "set_world"), make(M)) for M in sizes]
    times, probs = {name: [] for name, _ in legs}, {}
    for it in range(args.warm + args.reps):
        for name, (c, run) in legs:
            c.set_seed(0x5EED0001)                        # every leg, every repeat: the same runs
            t0 = time.perf_counter()
            p = run()
            dt = time.perf_counter() - t0
            if it >= args.warm:
                times[name].append(dt * 1e3)
            assert probs.setdefault(name[:3], p) == p, (name, p, probs)      # clutter out of reach changes no bit
    out = ["wall time of one call; %d alternating repeats after %d warm-up calls; %s" % (args.reps, args.warm, legs[0][1][0].lib.pocs_version().decode())]
    for name, (c, _) in legs:
        t = sorted(times[name])
        extra = ""
        if name.startswith("gmm") and c.world_boxes() > 64:
            extra = "   boxes in reach per waypoint: max %d" % int(c.world_reach().max())
        out.append("%-44s median %9.3f ms   min %9.3f   max %9.3f%s" % (name, statistics.median(t), t[0], t[-1], extra))
    out.append("probability of run 0, every leg: " + ", ".join("%s %.9f" % (k, v) for k, v in probs.items()))
    text = "\n".join(out)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    for _, (c, _) in legs:
        c.close()


if __name__ == "__main__":
    main()
