#!/usr/bin/env python3
"""What segment checks (pocs_set_segment_checks) cost a call.

Legs, one context each, ALTERNATING call by call: J = 1 (the default kernels) against J = 2, 4 and 8,
  gmm   bench.py's cfg2 at 20 runs per call: K = 3, 10^6 samples per run, samples stored (the default), the call as two
        sub-batches (the default at this size)
  mc    bench.py's cfg5 at 64 runs per call in the per-step form: 10^5 particles per run
on two scenes each:
  room     the bundled plan (gmm: its 56 waypoints; mc: resampled to 500) in the bundled room: little is in the way of any
           segment, so the GMM form's empty-list branch and the MC form's segment broad phase should carry it
  scene A  tests/test_segment_checks.py's scene at the same N: six waypoints 0.3 .. 0.9 m apart, the room's first three boxes and
           a post beside the middle of segment 1 -> 2, where about half of the belief collides on the way
With --parent DIR (a checkout of the parent commit, built) the J = 1 legs also alternate with the parent's library: expect no
difference beyond the spread of the parent against itself, which is measured too (two parent contexts).
Timed: the wall time of one pocs_run_gmm_estimation / pocs_run_simulation call (host chains, upload, graph replay, read-back: the
call ends in a device synchronise).  Median, min and max of the repeats in ms, and the ratio of the medians to the scene's J = 1.

  python tools/segment_checks_probe.py [--reps 15] [--warm 4] [--only gmm|mc] [--parent DIR] [--out FILE]
"""
import argparse
import importlib.util
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import pocs_amd  # noqa: E402

WPS = [1, 4, 10, 16, 18, 22]


def load_parent(path):
    """The parent commit's package, imported under another name from its own directory (its own libpocs.so)."""
    pkg = Path(path) / "probability-of-collision-for-safe-planning_amd"
    spec = importlib.util.spec_from_file_location("pocs_parent", pkg / "__init__.py", submodule_search_locations=[str(pkg)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["pocs_parent"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--only", default=None, choices=["gmm", "mc"])
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    plan, env = pocs_amd.load_plan(), pocs_amd.load_env()
    long_plan = pocs_amd.resample_plan(plan, 500)
    traj = np.asarray(plan["traj"], dtype=np.float64)[WPS].copy()
    plan_a = dict(traj=traj, odom=np.asarray(pocs_amd.planio.path_odometry(traj)).reshape(-1, 3))
    boxes_a = np.vstack([np.asarray(env["boxes"], dtype=np.float64).reshape(-1, 5)[:3], [0.5 * (traj[1, 0] + traj[2, 0]), -0.99, 0.02, 0.02, 0.3]])
    env_a = dict(footprint=env["footprint"], boxes=boxes_a)

    def gmm(mod, pl, ev, J):
        c = mod.Context(0)
        c.configure(pl, ev, K=3, N=1000000, seed=0x5EED0001)
        c.set_batch(20)
        if J > 1:
            c.set_segment_checks(J)
        return c, c.run_gmm_estimation

    def mc(mod, pl, ev, J):
        c = mod.Context(0)
        c.configure(pl, ev, K=1, N=100000, seed=0x5EED0001)
        c.set_batch(64)
        c.set_option(mod.OPT_MC_FUSED, 0)
        if J > 1:
            c.set_segment_checks(J)
        return c, c.run_simulation

    parent = load_parent(args.parent) if args.parent else None
    legs = []
    for kind, make, room_plan in (("gmm cfg2 x20", gmm, plan), ("mc cfg5 x64 per-step", mc, long_plan)):
        if args.only not in (None, kind.split()[0]):
            continue
        if parent is not None:
            legs += [("%s, room, parent" % kind, make(parent, room_plan, env, 1)), ("%s, room, parent again" % kind, make(parent, room_plan, env, 1))]
        legs += [("%s, room, J = %d" % (kind, J), make(pocs_amd, room_plan, env, J)) for J in (1, 2, 4, 8)]
        legs += [("%s, scene A, J = %d" % (kind, J), make(pocs_amd, plan_a, env_a, J)) for J in (1, 2, 4, 8)]
    times, probs = {name: [] for name, _ in legs}, {}
    for it in range(args.warm + args.reps):
        for name, (c, run) in legs:
            t0 = time.perf_counter()
            p = run()
            dt = time.perf_counter() - t0
            if it >= args.warm:
                times[name].append(dt * 1e3)
            probs[name] = p
    try:
        commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "no git"
    except OSError:
        commit = "no git"
    out = ["wall time of one call; %d alternating repeats after %d warm-up calls; %s; tree at %s; one MI355X"
           % (args.reps, args.warm, legs[0][1][0].lib.pocs_version().decode(), commit)]
    base = {}
    for name, _ in legs:
        t = sorted(times[name])
        med = statistics.median(t)
        key = ", ".join(name.split(", ")[:2])
        if name.endswith("J = 1"):
            base[key] = med
        ref = base.get(key)
        if "parent" in name:
            ref = None
        out.append("%-40s median %9.3f ms   min %9.3f   max %9.3f   %s   (p of last call %.6f)"
                   % (name, med, t[0], t[-1], ("x %.3f of J = 1" % (med / ref)) if ref else " " * 16, probs[name]))
    if parent is not None:
        for kind in sorted({n.split(", ")[0] for n, _ in legs}):
            p0 = statistics.median(times[kind + ", room, parent"]); p1 = statistics.median(times[kind + ", room, parent again"])
            j1 = statistics.median(times[kind + ", room, J = 1"])
            out.append("%s: J = 1 / parent x %.4f; parent again / parent x %.4f" % (kind, j1 / p0, p1 / p0))
    text = "\n".join(out)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    for _, (c, _) in legs:
        c.close()


if __name__ == "__main__":
    main()
