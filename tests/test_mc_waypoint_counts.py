"""First collisions per waypoint of Monte-Carlo calls (POCS_OPT_MC_WAYPOINT_COUNTS, pocs_mc_get_waypoint_counts) and the risk
bound obeyed by MC calls of plans (POCS_OPT_MC_RISK_BOUND).

F[w] = the shard's particles that collide at waypoint w and at no waypoint before it; C[s] = F[0] + ... + F[s].  Every expected
value comes from the CPU oracle alone.  The oracle has no per-waypoint MC output and needs none: its host chain is keyed by the
step index and its particles by their global index, so `orc.run_mc` on the prefix of length E of a plan gives every particle's
hit counter after waypoints 0 .. E - 1; run for E = 1 .. W it gives, per particle, the first waypoint at which the counter
leaves 0 (`prefix_profile`, which also checks that the prefixes are consistent: a counter grows by 0 or 1 per added waypoint).
The stop rule -- plan p stops at the FIRST waypoint s with float(C[s]) / float(N) >= bound, if s is not its last -- is a few
lines of Python over that profile (`stop_of`).  Every comparison is `==`.

With the eight candidates of tests/test_plan_risk_bound.py (lengths 20, 56, 1, 33, 2, 56', 7, 120; plan p on the stream of run
p; K = 1) the oracle gives, at bound 0.2, as the first s with C[s] / N >= 0.2 (-: never), at N = 3001 and at N = 20000 alike:

    p0   p1   p2   p3   p4   p5   p6   p7
    16   34    -    8    -   34    -   16

so five plans stop strictly before their end and three never reach the bound; `conditions` asserts what makes a pass
meaningful from the oracle's values inside the test.

The CPU tests check the declarations and the prefix oracle's self-consistency; everything that launches is marked `gpu`."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest

from test_plan_risk_bound import BOUND, LENGTHS, SEED, candidates, prefix, seed_of

ROOT = Path(__file__).resolve().parents[1]
K = 1                                       # the MC path does not depend on the number of Gaussians
ORACLE_STOPS = [16, 34, None, 8, None, 34, None, 16]

_profiles = {}


def prefix_profile(orc, pl, env, seed, N, first=0, count=None, key=None):
    """(F uint64[W], the particles' hit counters after the whole plan) of particles [first, first + count) from the oracle's
    runs of the plan's prefixes."""
    count = N if count is None else count
    k = None if key is None else (key, seed, N, first, count)
    if k in _profiles:
        return _profiles[k]
    W = len(np.asarray(pl["traj"]))
    prev, F = np.zeros(count, np.int64), []
    for E in range(1, W + 1):
        n, hits, _ = orc.run_mc(orc.config(prefix(pl, E), env, K=K), seed, N, first, count)
        hits = hits.astype(np.int64)
        grew = hits - prev
        assert ((grew == 0) | (grew == 1)).all(), E          # the prefix of length E - 1 is the head of the prefix of length E
        F.append(int(((prev == 0) & (hits > 0)).sum()))
        assert n == int((hits > 0).sum()) == sum(F), E       # the prefix's collided count is sum F
        prev = hits
    out = (np.array(F, dtype=np.uint64), prev.astype(np.uint32))
    if k is not None:
        _profiles[k] = out
    return out


def stop_of(F, N, bound):
    """The stop rule over a profile: dict(s, E, count, prob, c) -- s the first waypoint with C[s] / N >= bound (None: never),
    E the waypoints evaluated, count and prob what the plan reports."""
    Cs = np.cumsum(F.astype(np.int64)).tolist()
    c = [float(v) / float(N) for v in Cs]
    W = len(Cs)
    s = next((w for w, cw in enumerate(c) if cw >= bound), None) if bound < 1.0 else None
    cut = s is not None and s + 1 < W
    E = s + 1 if cut else W
    return dict(s=s, W=W, E=E, count=Cs[E - 1], prob=float(Cs[E - 1]) / float(N), c=c)


def conditions(exps, bound):
    """What makes a pass meaningful, from the oracle's values alone."""
    stopped = [p for p, e in enumerate(exps) if e["E"] < e["W"]]
    never = [p for p, e in enumerate(exps) if e["s"] is None]
    assert len(stopped) >= 2 and len(never) >= 2, (stopped, never)
    order = sorted(range(len(exps)), key=lambda p: -exps[p]["W"])           # slot order: descending length, ties in plan order
    assert any((a in stopped) != (b in stopped) for a, b in zip(order, order[1:])), order      # a stopped next to a live plan
    for e in exps:
        for cw in e["c"]:
            assert abs(cw - bound) > 4 * math.ulp(bound), (cw, bound)      # the specification does not care about a tie
    return stopped, never


def plan_profiles(orc, pocs, plan, env, N, common_seed=False):
    plans = candidates(pocs, plan)
    return plans, [prefix_profile(orc, pl, env, seed_of(0 if common_seed else p), N, key=("cand", p)) for p, pl in enumerate(plans)]


# ---- CPU -----------------------------------------------------------------------------------------------------------

def test_waypoint_counts_are_declared_and_wrapped(pocs):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pocs.h").read_text(), flags=re.S)
    assert re.search(r"int\s+pocs_mc_get_waypoint_counts\s*\(\s*pocs_ctx\s*\*\s*ctx\s*,\s*unsigned\s+long\s+long\s*\*\s*out\s*,\s*int\s+cap\s*\)\s*;", text)
    assert re.search(r"#define\s+POCS_OPT_MC_WAYPOINT_COUNTS\s+11\b", text) and re.search(r"#define\s+POCS_OPT_MC_RISK_BOUND\s+12\b", text)
    assert pocs.SIGNATURES["pocs_mc_get_waypoint_counts"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_int])
    assert (pocs.OPT_MC_WAYPOINT_COUNTS, pocs.OPT_MC_RISK_BOUND) == (11, 12)
    assert callable(pocs.Context.mc_waypoint_counts)


@pytest.mark.parametrize("N", [3001, 20000])
def test_prefix_oracle_is_consistent(pocs, orc, plan, env, N):
    """The oracle side alone: consistent prefixes (inside prefix_profile), the stops of the table above, profiles that
    exercise the initial cloud and many waypoints, and shards that add up."""
    plans, profs = plan_profiles(orc, pocs, plan, env, N)
    exps = [stop_of(F, N, BOUND) for F, _ in profs]
    print("N %d  first s with C[s]/N >= %g: %s" % (N, BOUND, [e["s"] for e in exps]))
    stopped, never = conditions(exps, BOUND)
    assert [e["s"] for e in exps] == ORACLE_STOPS
    assert len(stopped) == 5 and len(never) == 3
    for p, (F, hits) in enumerate(profs):
        assert len(F) == LENGTHS[p] and F[0] > 0
        n, _, _ = orc.run_mc(orc.config(plans[p], env, K=K), seed_of(p), N)
        assert int(F.sum()) == n == int((hits > 0).sum()), p
        if p in stopped:
            assert 10 <= int((F > 0).sum()) <= 32, (p, int((F > 0).sum()))
    if N == 3001:
        whole, _ = prefix_profile(orc, plan, env, seed_of(0), N, key="bundled")
        lo, _ = prefix_profile(orc, plan, env, seed_of(0), N, 0, 1000, key="bundled")
        hi, _ = prefix_profile(orc, plan, env, seed_of(0), N, 1000, 2001, key="bundled")
        assert np.array_equal(lo + hi, whole) and lo.sum() > 0 and hi.sum() > 0


# ---- GPU -----------------------------------------------------------------------------------------------------------

def mc_context(pocs, plan, env, N, counts=1, seed=SEED):
    c = pocs.Context(0)
    c.configure(plan, env, K=K, N=N, seed=seed)
    c.set_option(pocs.OPT_MC_WAYPOINT_COUNTS, counts)
    return c


@pytest.mark.gpu
def test_profile_of_single_batched_and_served_runs(pocs, orc, plan, env):
    N = 3001
    want = [prefix_profile(orc, plan, env, seed_of(r), N, key="bundled")[0] for r in range(4)]
    with mc_context(pocs, plan, env, N) as c:
        p = c.run_simulation()                               # a single run
        F = c.mc_waypoint_counts()
        print("single run: F %s" % F.tolist())
        assert F.dtype == np.uint64 and np.array_equal(F, want[0])
        assert int(F.sum()) == c.mc_batch_counts()[0] and p == int(F.sum()) / N
        c.set_batch(3)                                       # runs 1, 2, 3 of the context
        c.run_simulation()
        counts = c.mc_batch_counts()
        for r in range(3):
            c.select_batch_run(r)
            F = c.mc_waypoint_counts()
            assert np.array_equal(F, want[1 + r]) and int(F.sum()) == counts[r], r
    with mc_context(pocs, plan, env, N) as c:                # run-ahead: four runs in one launch, served one per call
        c.set_option(pocs.OPT_RUN_AHEAD, 4)
        for r in range(4):
            p = c.run_simulation()
            F = c.mc_waypoint_counts()
            assert np.array_equal(F, want[r]), r
            assert c.mc_batch_counts() == [int(F.sum())] and p == int(F.sum()) / N, r


@pytest.mark.gpu
def test_launch_forms_give_the_same_profile(pocs, orc, plan, env):
    N = 3001
    want, _ = prefix_profile(orc, plan, env, seed_of(0), N, key="bundled")
    with mc_context(pocs, plan, env, N) as c:
        for fused in (0, 1):
            for nt in (0, 1):
                for graph in (1, 0):
                    c.set_option(pocs.OPT_MC_FUSED, fused)
                    c.set_option(pocs.OPT_MC_NONTEMPORAL, nt)
                    c.set_option(pocs.OPT_USE_GRAPH, graph)
                    for _ in range(2):                       # (graph: captured, then replayed)
                        c.set_seed(SEED)
                        c.run_simulation()
                        F = c.mc_waypoint_counts()
                        assert np.array_equal(F, want), (fused, nt, graph)
                        assert c.mc_batch_counts() == [int(want.sum())]


@pytest.mark.gpu
def test_profiles_of_a_plan_batch(pocs, orc, plan, env):
    N = 3001
    plans, profs = plan_profiles(orc, pocs, plan, env, N)
    with mc_context(pocs, plan, env, N) as c:
        c.set_plans(plans)
        for fused in (0, 1):
            c.set_option(pocs.OPT_MC_FUSED, fused)
            c.set_seed(SEED)
            c.run_simulation()
            counts = c.mc_batch_counts()
            assert c.plan_evaluated().tolist() == list(LENGTHS)
            for p, (F, _) in enumerate(profs):
                c.select_batch_run(p)
                got = c.mc_waypoint_counts()
                assert len(got) == LENGTHS[p] and np.array_equal(got, F), (fused, p)
                assert counts[p] == int(F.sum()), (fused, p)


@pytest.mark.gpu
def test_shard_profiles_add_up(pocs, orc, plan, env):
    N = 3001
    whole, _ = prefix_profile(orc, plan, env, seed_of(0), N, key="bundled")
    got = []
    with mc_context(pocs, plan, env, N) as c:
        for first, count in ((0, 1000), (1000, 2001)):
            want, _ = prefix_profile(orc, plan, env, seed_of(0), N, first, count, key="bundled")
            c.set_shard(first, count)
            c.set_seed(SEED)
            n = c.mc_run_local()
            F = c.mc_waypoint_counts()
            assert np.array_equal(F, want) and n == int(want.sum()), (first, count)
            got.append(F)
    assert np.array_equal(got[0] + got[1], whole)


@pytest.mark.gpu
def test_larger_runs_where_blocks_and_grid_strides_matter(pocs, orc, plan, env):
    short = prefix(plan, 20)
    N = 200000
    want, _ = prefix_profile(orc, short, env, seed_of(0), N)
    with mc_context(pocs, short, env, N) as c:
        for fused in (0, 1):
            c.set_option(pocs.OPT_MC_FUSED, fused)
            c.set_seed(SEED)
            c.run_simulation()
            F = c.mc_waypoint_counts()
            print("N %d fused %d: F %s" % (N, fused, F.tolist()))
            assert np.array_equal(F, want), fused
    N = 10**6
    n, _, _ = orc.run_mc(orc.config(short, env, K=K), seed_of(0), N)
    with mc_context(pocs, short, env, N) as c:
        both = []
        for fused in (0, 1):
            c.set_option(pocs.OPT_MC_FUSED, fused)
            c.set_seed(SEED)
            c.run_simulation()
            both.append(c.mc_waypoint_counts().copy())
            assert int(both[-1].sum()) == n == c.mc_batch_counts()[0], fused
        assert np.array_equal(both[0], both[1]) and (both[0] > 0).sum() >= 10


def check_stopped_call(c, pocs, orc, plans, env, profs, exps, N, seeds, p0):
    E, counts, probs = c.plan_evaluated(), c.mc_batch_counts(), c.batch_probabilities()
    print("N %d  E %s  oracle %s  counts %s" % (N, E.tolist(), [e["E"] for e in exps], counts))
    assert E.tolist() == [e["E"] for e in exps]
    assert counts == [e["count"] for e in exps]
    assert probs.tolist() == [e["prob"] for e in exps] and p0 == probs[0]
    for p, (e, (F, _)) in enumerate(zip(exps, profs)):
        c.select_batch_run(p)
        got = c.mc_waypoint_counts()
        assert len(got) == e["E"] and np.array_equal(got, F[:e["E"]]), p
        assert c.path_length() == e["W"], p
        if e["E"] < e["W"]:
            assert probs[p] >= BOUND and e["c"][e["E"] - 1] == probs[p], p


@pytest.mark.gpu
@pytest.mark.parametrize("N", [3001, 20000])
def test_mc_stop_matches_the_oracle(pocs, orc, plan, env, N):
    plans, profs = plan_profiles(orc, pocs, plan, env, N)
    exps = [stop_of(F, N, BOUND) for F, _ in profs]
    stopped, never = conditions(exps, BOUND)
    with mc_context(pocs, plan, env, N, counts=0) as c:
        c.set_plans(plans)
        c.set_plan_risk_bound(BOUND)
        c.set_option(pocs.OPT_MC_RISK_BOUND, 1)
        for fused in (0, 1):                                 # the stop takes the per-step form whatever OPT_MC_FUSED says
            c.set_option(pocs.OPT_MC_FUSED, fused)
            for _ in range(2):                               # captured, then replayed
                c.set_seed(SEED)
                p0 = c.run_simulation()
                check_stopped_call(c, pocs, orc, plans, env, profs, exps, N, None, p0)
        c.set_option(pocs.OPT_MC_FUSED, 0)
        # a stopped plan's cloud is the one at its stop, its hit counters cover waypoints 0 .. s
        p = stopped[0]
        e = exps[p]
        _, hits, parts = orc.run_mc(orc.config(prefix(plans[p], e["E"]), env, K=K), seed_of(p), N, want_particles=True)
        c.select_batch_run(p)
        xyz, got_hits = c.particles(N)
        assert np.array_equal(got_hits, hits) and np.array_equal(xyz, parts), p
        assert int((got_hits > 0).sum()) == e["count"]
        # a changed bound: captured again
        other = 0.1
        exps2 = [stop_of(F, N, other) for F, _ in profs]
        assert [x["E"] for x in exps2] != [x["E"] for x in exps]
        for x in exps2:
            for cw in x["c"]:
                assert abs(cw - other) > 4 * math.ulp(other)
        c.set_plan_risk_bound(other)
        c.set_seed(SEED)
        c.run_simulation()
        assert c.plan_evaluated().tolist() == [x["E"] for x in exps2] and c.mc_batch_counts() == [x["count"] for x in exps2]
        if N == 3001:                                        # common random numbers: every plan on the stream of run 0
            _, profs0 = plan_profiles(orc, pocs, plan, env, N, common_seed=True)
            exps0 = [stop_of(F, N, BOUND) for F, _ in profs0]
            assert any(x["E"] < x["W"] for x in exps0)
            c.set_plan_risk_bound(BOUND)
            c.set_option(pocs.OPT_PLAN_SEEDS, 1)
            c.set_seed(SEED)
            p0 = c.run_simulation()
            check_stopped_call(c, pocs, orc, plans, env, profs0, exps0, N, None, p0)


@pytest.mark.gpu
def test_stop_option_without_a_bound_or_without_plans_changes_nothing(pocs, orc, plan, env):
    N = 3001
    plans, profs = plan_profiles(orc, pocs, plan, env, N)
    full = [stop_of(F, N, 1.0) for F, _ in profs]
    assert [e["E"] for e in full] == list(LENGTHS)
    out = (C.c_ulonglong * 256)()
    with mc_context(pocs, plan, env, N, counts=1) as c:
        c.set_option(pocs.OPT_MC_RISK_BOUND, 1)
        c.set_plans(plans)                                   # the option on, the bound off
        p0 = c.run_simulation()
        check_stopped_call(c, pocs, orc, plans, env, profs, full, N, None, p0)
        c.set_plan_risk_bound(7.5)
        c.set_seed(SEED)
        p0 = c.run_simulation()
        check_stopped_call(c, pocs, orc, plans, env, profs, full, N, None, p0)
        c.clear_plans()                                      # the option on, a bound set, no plans
        c.set_plan_risk_bound(BOUND)
        want, _ = prefix_profile(orc, plan, env, seed_of(0), N, key="bundled")
        assert stop_of(want, N, BOUND)["E"] < 56             # (as a plan of a batch it would stop)
        for fused in (0, 1):
            c.set_option(pocs.OPT_MC_FUSED, fused)
            c.set_seed(SEED)
            p = c.run_simulation()
            F = c.mc_waypoint_counts()
            assert np.array_equal(F, want) and p == int(want.sum()) / N and c.mc_batch_counts() == [int(want.sum())]
        # option 0 after option 1: the next MC call leaves no profile -- with the stop option still on but idle ...
        c.set_option(pocs.OPT_MC_WAYPOINT_COUNTS, 0)
        c.set_seed(SEED)
        assert c.run_simulation() == int(want.sum()) / N
        assert c.lib.pocs_mc_get_waypoint_counts(c.h, out, 256) == -3
        # ... and a stopped call has one, whatever OPT_MC_WAYPOINT_COUNTS says, until the stop option goes too
        c.set_plans(plans)
        c.set_seed(SEED)
        c.run_simulation()
        exps = [stop_of(F, N, BOUND) for F, _ in profs]
        assert c.plan_evaluated().tolist() == [e["E"] for e in exps]
        c.select_batch_run(3)
        assert np.array_equal(c.mc_waypoint_counts(), profs[3][0][:exps[3]["E"]])
        c.set_option(pocs.OPT_MC_RISK_BOUND, 0)
        c.set_seed(SEED)
        c.run_simulation()
        assert c.plan_evaluated().tolist() == list(LENGTHS) and c.mc_batch_counts() == [e["count"] for e in full]
        assert c.lib.pocs_mc_get_waypoint_counts(c.h, out, 256) == -3


@pytest.mark.gpu
def test_refusals(pocs, orc, plan, env):
    N = 3001
    out = (C.c_ulonglong * 64)()
    with mc_context(pocs, plan, env, N) as c:
        lib, h = c.lib, c.h
        assert lib.pocs_mc_get_waypoint_counts(h, out, 64) == -3          # before any call
        c.run_simulation()
        assert lib.pocs_mc_get_waypoint_counts(h, out, 55) == -6          # 56 waypoints
        assert lib.pocs_mc_get_waypoint_counts(h, None, 64) == -1
        assert lib.pocs_mc_get_waypoint_counts(h, out, 56) == 56
        want, _ = prefix_profile(orc, plan, env, seed_of(0), N, key="bundled")
        assert list(out[:56]) == want.tolist()
        c.run_gmm_estimation()
        assert lib.pocs_mc_get_waypoint_counts(h, out, 64) == -3          # the last call was not an MC call
        assert "MC call" in lib.pocs_last_error(h).decode()
        for bad in (-1, 2):
            assert lib.pocs_set_option(h, pocs.OPT_MC_WAYPOINT_COUNTS, bad) == -1
            assert lib.pocs_set_option(h, pocs.OPT_MC_RISK_BOUND, bad) == -1
