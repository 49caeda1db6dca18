"""A risk bound for calls of candidate plans (pocs_set_plan_risk_bound): a plan whose running probability
c_w = 1 - prod_{v <= w} (1 - p_v) has reached the bound is not evaluated any further, and pocs_get_plan_evaluated tells
where it stopped.  Everything expected here comes from the CPU oracle run on each plan ALONE and to its end -- the stop
rule is a few lines of float64 Python over the oracle's waypoint probabilities (`expected`) --, never from the library
with the bound off.  Every comparison is exact.

The bound of the oracle tests is 0.2 for each (K, N).  With the eight candidates of tests/test_plan_batches.py (lengths
20, 56, 1, 33, 2, 56', 7, 120; plan p on the stream of run p) the oracle alone gives, as the first waypoint s with
c_s >= 0.2 per plan (-: never):

    (K, N)       p0   p1   p2   p3   p4   p5   p6   p7
    (1, 3001)     -   34    -   20    -   34    -   72
    (3, 5000)     -   34    -   19    -   34    -   72
    (8, 2048)     -   34    -   20    -   34    -   67

so four plans stop strictly before their last waypoint, four never reach the bound, and in slot order (descending
length: 7, 1, 5, 3, 0, 6, 4, 2) the stopped plan 3 sits next to the live plan 0.  `conditions` asserts all of that, and
that no c_w lies within 4 ulp of the bound, from the oracle's values inside the test.

The CPU test checks the declarations; everything that launches is marked `gpu`."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest

SEED = 0x5EED0001
WEYL = 0x9E3779B97F4A7C15            # effective seed of the r-th run of a context = seed + r * WEYL (mod 2^64)
ROOT = Path(__file__).resolve().parents[1]
LENGTHS = (20, 56, 1, 33, 2, 56, 7, 120)      # as tests/test_plan_batches.py
BOUND = 0.2


def seed_of(r):
    return (SEED + r * WEYL) % 2**64


def shifted(pocs, plan, dy):
    traj = np.asarray(plan["traj"]) + np.array([0.0, dy, 0.0])
    return dict(traj=traj, odom=pocs.planio.path_odometry(traj))


def prefix(plan, W):
    return dict(traj=np.asarray(plan["traj"])[:W].copy(), odom=np.asarray(plan["odom"])[:W - 1].copy().reshape(-1, 3))


def candidates(pocs, plan, lengths=LENGTHS):
    """tests/test_plan_batches.py::candidates, restated: prefixes of the bundled plan (W = 56), resampled copies (other
    lengths) and a laterally shifted copy (the second 56)."""
    out, seen56 = [], False
    for W in lengths:
        if W == 56 and seen56:
            out.append(shifted(pocs, plan, 0.1))
        elif W <= 56 and W not in (33,):
            out.append(prefix(plan, W))
        else:
            out.append(pocs.resample_plan(plan, W))
        seen56 = seen56 or W == 56
    return out


def expected(orc, pl, env, K, seed, N, bound):
    """The oracle's full run of the plan alone, and the stop rule over its waypoint probabilities."""
    cfg = orc.config(pl, env, K=K)
    want = orc.run_gmm(cfg, seed, N)
    prod, c = 1.0, []
    for p_w in want["probs"]:
        prod *= (1.0 - float(p_w))
        c.append(1.0 - prod)
    assert c[-1] == want["prob"]                    # the restated rule IS the oracle's own combine
    s = next((w for w, cw in enumerate(c) if cw >= bound), None) if bound < 1.0 else None
    W = len(c)
    return dict(cfg=cfg, want=want, c=c, s=s, W=W, E=(s + 1 if s is not None else W),
                prob=(c[s] if s is not None else want["prob"]))


def conditions(exps, bound):
    """What makes a pass meaningful, from the oracle's values alone."""
    stopped = [p for p, e in enumerate(exps) if e["s"] is not None and e["s"] + 1 < e["W"]]
    never = [p for p, e in enumerate(exps) if e["s"] is None]
    assert len(stopped) >= 2 and len(never) >= 2, (stopped, never)
    order = sorted(range(len(exps)), key=lambda p: -exps[p]["W"])           # slot order: descending length, ties in plan order
    assert any((a in stopped) != (b in stopped) and (a in stopped or b in stopped) and (a in never or b in never)
               for a, b in zip(order, order[1:])), order
    for e in exps:
        for cw in e["c"]:
            assert abs(cw - bound) > 4 * math.ulp(bound), (cw, bound)      # the specification does not care about a tie
    return stopped, never


def view(c, p, K, states_at=None):
    """What the getters show of plan p: its evaluated waypoints."""
    c.select_batch_run(p)
    E = int(c.plan_evaluated()[p])
    probs = c.waypoint_probabilities().copy()
    out = dict(E=E, W=c.path_length(), probs=probs, moments=np.array([c.moments(w, K) for w in range(E)]))
    ws = sorted({0, E // 2, E - 1}) if states_at is None else states_at
    out["states"] = {w: c.gmm_state_raw(w, K)[..., :14] for w in ws}
    return out


def check_plan(c, pocs, p, e, K):
    got = view(c, p, K)
    assert got["W"] == e["W"], p                                            # pocs_get_path_length stays W[p]
    assert got["E"] == e["E"], (p, got["E"], e["E"])
    assert len(got["probs"]) == e["E"] and np.array_equal(got["probs"], e["want"]["probs"][:e["E"]]), p
    assert np.array_equal(got["moments"], e["want"]["moments"][:e["E"]]), p
    for w, s in got["states"].items():
        assert np.array_equal(s, e["want"]["states"][w][..., :14]), (p, w)
    for getter in (c.moments, c.gmm_state):                                  # nothing past the last evaluated waypoint
        with pytest.raises(pocs.PocsError) as err:
            getter(e["E"], K)
        assert err.value.code == -1, p


def flat(c, n, K):
    """Everything a call of n plans returned, as a list to compare two calls by."""
    out = [c.plan_evaluated().copy(), c.batch_probabilities().copy()]
    for p in range(n):
        v = view(c, p, K)
        out += [v["probs"], v["moments"]] + [v["states"][w] for w in sorted(v["states"])]
    return out


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- CPU -----------------------------------------------------------------------------------------------------------

def test_risk_bound_is_declared_and_wrapped(pocs):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pocs.h").read_text(), flags=re.S)
    assert re.search(r"int\s+pocs_set_plan_risk_bound\s*\(\s*pocs_ctx\s*\*\s*ctx\s*,\s*double\s+bound\s*\)\s*;", text)
    assert re.search(r"int\s+pocs_get_plan_evaluated\s*\(\s*pocs_ctx\s*\*\s*ctx\s*,\s*int\s*\*\s*out\s*,\s*int\s+cap\s*\)\s*;", text)
    assert pocs.SIGNATURES["pocs_set_plan_risk_bound"] == (C.c_int, [C.c_void_p, C.c_double])
    assert pocs.SIGNATURES["pocs_get_plan_evaluated"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int])
    assert callable(pocs.Context.set_plan_risk_bound) and callable(pocs.Context.plan_evaluated)


# ---- GPU -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx(pocs):
    c = pocs.Context(0)
    yield c
    c.close()


def configured(c, pocs, plan, env, plans, K, N, bound, seed=SEED):
    if getattr(c, "_single_batch", None) is not None:
        c.clear_plans()
    c.configure(plan, env, K=K, N=N, seed=seed)
    c.set_plans(plans)
    c.set_plan_risk_bound(bound)


@pytest.mark.gpu
@pytest.mark.parametrize("K,N", [(1, 3001), (3, 5000), (8, 2048)])
def test_stopped_and_unstopped_plans_match_the_oracle(ctx, pocs, orc, plan, env, K, N):
    plans = candidates(pocs, plan)
    exps = [expected(orc, pl, env, K, seed_of(p), N, BOUND) for p, pl in enumerate(plans)]
    stopped, never = conditions(exps, BOUND)
    configured(ctx, pocs, plan, env, plans, K, N, BOUND)
    try:
        p0 = ctx.run_gmm_estimation()
        E, finals = ctx.plan_evaluated(), ctx.batch_probabilities()
        print("K %d N %d  E %s  oracle %s  finals %s" % (K, N, E.tolist(), [e["E"] for e in exps], finals.tolist()))
        assert E.dtype == np.int32 and E.tolist() == [e["E"] for e in exps]
        assert finals.tolist() == [e["prob"] for e in exps] and p0 == finals[0]
        for p in stopped:
            assert finals[p] >= BOUND and E[p] < exps[p]["W"]
        for p, e in enumerate(exps):
            check_plan(ctx, pocs, p, e, K)
        # the samples a stopped plan left are those of its last evaluated waypoint: the later launches drew nothing for it
        for p in stopped[:2] + never[:1]:
            e = exps[p]
            w = e["E"] - 1
            _, samples, flags, _ = orc.gmm_waypoint(e["cfg"], seed_of(p), w, e["want"]["states"][w], 0, N, want_samples=True)
            ctx.select_batch_run(p)
            xyz, got_flags = ctx.gmm_samples(N)
            assert np.array_equal(got_flags, flags) and np.array_equal(xyz, samples), p
    finally:
        ctx.set_plan_risk_bound(1.0)


@pytest.mark.gpu
def test_launch_forms_change_no_bit_and_no_stop(pocs, orc, plan, env):
    """Sub-batches 1 and 2, graph replay and eager launches, samples stored or not, the profiling form, both seed rules:
    the same stops and the same bits.  Then eight plans at a sample count where the default rule takes two sub-batches."""
    K, N = 3, 40001
    plans = candidates(pocs, plan)
    with pocs.Context(0) as c:
        c.configure(plan, env, K=K, N=N, seed=SEED)
        c.set_plans(plans)
        c.set_plan_risk_bound(BOUND)
        for crn in (0, 1):
            c.set_option(pocs.OPT_PLAN_SEEDS, crn)
            c.set_option(pocs.OPT_PROFILE, 0)
            outs = []
            for sub, graph, store in ((1, 1, 1), (2, 1, 1), (2, 0, 1), (1, 0, 0), (2, 1, 0), (2, 1, 1)):
                c.set_option(pocs.OPT_SUB_BATCHES, sub)
                c.set_option(pocs.OPT_USE_GRAPH, graph)
                c.set_option(pocs.OPT_STORE_SAMPLES, store)
                c.set_seed(SEED)
                c.run_gmm_estimation()
                outs.append(flat(c, len(plans), K))
            c.set_option(pocs.OPT_PROFILE, 1)
            c.set_seed(SEED)
            c.run_gmm_estimation()
            outs.append(flat(c, len(plans), K))
            for i, o in enumerate(outs[1:]):
                assert same(o, outs[0]), (crn, i + 1)
            exps = [expected(orc, pl, env, K, seed_of(0 if crn else p), N, BOUND) for p, pl in enumerate(plans)]
            assert outs[0][0].tolist() == [e["E"] for e in exps] and outs[0][1].tolist() == [e["prob"] for e in exps], crn
            assert any(e["E"] < e["W"] for e in exps) and any(e["s"] is None for e in exps)

        N = 160000                                       # 8 plans x 1.6e5 samples: two sub-batches by default
        c.set_option(pocs.OPT_PLAN_SEEDS, 0)
        c.set_option(pocs.OPT_PROFILE, 0)
        c.set_option(pocs.OPT_STORE_SAMPLES, 1)
        c.set_num_gmm_samples(N)
        big = []
        for sub in (0, 1):
            c.set_option(pocs.OPT_SUB_BATCHES, sub)
            c.set_option(pocs.OPT_USE_GRAPH, 1)
            c.set_seed(SEED)
            c.run_gmm_estimation()
            big.append(flat(c, len(plans), K) + list(c.gmm_samples(N)))
        assert same(big[1], big[0])
        for p in (0, 3, 7):
            e = expected(orc, plans[p], env, K, seed_of(p), N, BOUND)
            assert big[0][0][p] == e["E"] and big[0][1][p] == e["prob"], p
            check_plan(c, pocs, p, e, K)
        assert big[0][0][7] < 120 and big[0][0][0] == 20


@pytest.mark.gpu
def test_blocks_that_straddle_a_stopped_and_a_live_run(pocs, orc, plan, env):
    """Five plans of 262144 samples in ONE launch per waypoint: 256 virtual slices per run dealt three at a time, so a
    block's range crosses from one run into the next -- and in slot order the plans alternate between stopped (at waypoint
    0; around the middle) and live, so blocks meet a stopped first run with a live second one and the other way round."""
    K, N = 3, 262144
    up = shifted(pocs, plan, 0.05)
    plans = [shifted(pocs, plan, -0.05), up, plan, prefix(up, 48), prefix(plan, 44)]      # slot order = plan order
    exps = [expected(orc, pl, env, K, seed_of(p), N, BOUND) for p, pl in enumerate(plans)]
    conditions(exps, BOUND)
    assert [e["s"] is None for e in exps] == [False, True, False, True, False] and exps[0]["E"] == 1, [e["E"] for e in exps]
    with pocs.Context(0) as c:
        c.configure(plan, env, K=K, N=N, seed=SEED)
        c.set_plans(plans)
        c.set_plan_risk_bound(BOUND)
        c.set_option(pocs.OPT_SUB_BATCHES, 1)
        for _ in range(2):                               # captured, then replayed
            c.set_seed(SEED)
            c.run_gmm_estimation()
            print("E %s  oracle %s" % (c.plan_evaluated().tolist(), [e["E"] for e in exps]))
            assert c.plan_evaluated().tolist() == [e["E"] for e in exps]
            assert c.batch_probabilities().tolist() == [e["prob"] for e in exps]
            for p, e in enumerate(exps):
                check_plan(c, pocs, p, e, K)
        for p in (0, 2):                                 # the stopped plans' samples are those of their last waypoint
            e = exps[p]
            w = e["E"] - 1
            _, samples, flags, _ = orc.gmm_waypoint(e["cfg"], seed_of(p), w, e["want"]["states"][w], 0, N, want_samples=True)
            c.select_batch_run(p)
            xyz, got_flags = c.gmm_samples(N)
            assert np.array_equal(got_flags, flags) and np.array_equal(xyz, samples), p


@pytest.mark.gpu
def test_off_means_off(pocs, orc, plan, env):
    K, N = 3, 5000
    plans = candidates(pocs, plan, (56, 33, 20, 56))
    P = len(plans)
    full = lambda call: [expected(orc, pl, env, K, seed_of(call * P + p), N, 1.0) for p, pl in enumerate(plans)]
    cut = lambda call: [expected(orc, pl, env, K, seed_of(call * P + p), N, BOUND) for p, pl in enumerate(plans)]

    def check(c, exps):
        assert c.plan_evaluated().tolist() == [e["E"] for e in exps]
        assert c.batch_probabilities().tolist() == [e["prob"] for e in exps]
        for p, e in enumerate(exps):
            check_plan(c, pocs, p, e, K)

    with pocs.Context(0) as c:                           # a context that never set a bound
        c.configure(plan, env, K=K, N=N, seed=SEED)
        c.set_plans(plans)
        c.run_gmm_estimation()
        exps = full(0)
        assert [e["E"] for e in exps] == [56, 33, 20, 56]
        check(c, exps)
    with pocs.Context(0) as c:
        c.configure(plan, env, K=K, N=N, seed=SEED)
        c.set_plans(plans)
        c.set_plan_risk_bound(1.0)
        c.run_gmm_estimation()
        check(c, full(0))
        # on -> off -> on, every phase captured once and replayed once; the run counter advances by P per call
        call = 1
        for bound, exp_of in ((BOUND, cut), (1.0, full), (7.5, full), (BOUND, cut)):
            c.set_plan_risk_bound(bound)
            for _ in range(2):
                c.run_gmm_estimation()
                exps = exp_of(call)
                if bound < 1.0:
                    assert sum(e["E"] < e["W"] for e in exps) >= 2
                check(c, exps)
                call += 1
        # the bound survives a new set of plans
        c.set_plans(plans[:3])
        c.set_seed(SEED)
        c.run_gmm_estimation()
        exps = [expected(orc, pl, env, K, seed_of(p), N, BOUND) for p, pl in enumerate(plans[:3])]
        assert exps[0]["E"] < 56
        check(c, exps)


@pytest.mark.gpu
def test_one_plan_stops_as_it_does_in_a_batch(pocs, orc, plan, env):
    K, N = 3, 30000
    e = expected(orc, plan, env, K, seed_of(0), N, BOUND)
    assert e["s"] is not None and 1 < e["E"] < 56
    with pocs.Context(0) as c:
        c.configure(plan, env, K=K, N=N, seed=SEED)
        c.set_plans([plan])
        c.set_plan_risk_bound(BOUND)
        for _ in range(2):
            c.set_seed(SEED)
            p = c.run_gmm_estimation()
            assert p == e["prob"] and c.batch_probabilities().tolist() == [e["prob"]] and c.plan_evaluated().tolist() == [e["E"]]
            check_plan(c, pocs, 0, e, K)
        alone = view(c, 0, K, states_at=list(range(e["E"])))
        _, samples, flags, _ = orc.gmm_waypoint(e["cfg"], seed_of(0), e["E"] - 1, e["want"]["states"][e["E"] - 1], 0, N, want_samples=True)
        xyz, got_flags = c.gmm_samples(N)
        assert np.array_equal(got_flags, flags) and np.array_equal(xyz, samples)
        # as one of several, under common random numbers (every plan on run 0's stream)
        c.set_plans([prefix(plan, 20), plan, shifted(pocs, plan, 0.1)])
        c.set_option(pocs.OPT_PLAN_SEEDS, 1)
        c.set_seed(SEED)
        c.run_gmm_estimation()
        assert c.plan_evaluated()[1] == e["E"] and c.batch_probabilities()[1] == e["prob"]
        among = view(c, 1, K, states_at=list(range(e["E"])))
        assert np.array_equal(among["probs"], alone["probs"]) and np.array_equal(among["moments"], alone["moments"])
        assert all(np.array_equal(among["states"][w], alone["states"][w]) for w in range(e["E"]))


@pytest.mark.gpu
def test_a_later_call_is_clean(pocs, orc, plan, env):
    K, N = 3, 6000
    plans = candidates(pocs, plan, (20, 56, 7, 33))

    def single(c):
        return [np.float64(c.run_gmm_estimation()), c.waypoint_probabilities().copy(),
                np.array([c.moments(w, K) for w in range(56)]), np.array([c.gmm_state_raw(w, K) for w in range(56)])]

    with pocs.Context(0) as c:
        c.configure(plan, env, K=K, N=N, seed=SEED)
        c.set_plans(plans)
        c.set_plan_risk_bound(BOUND)
        c.run_gmm_estimation()
        assert (c.plan_evaluated() < np.array([20, 56, 7, 33])).sum() >= 2
        c.clear_plans()                                  # (the bound stays set: it has no effect without plans)
        assert c.path_length() == 56
        c.set_seed(SEED)
        got = single(c)
        assert len(c.batch_probabilities()) == 1
        with pytest.raises(pocs.PocsError) as err:
            c.plan_evaluated()
        assert err.value.code == -3
    with pocs.Context(0) as f:
        f.configure(plan, env, K=K, N=N, seed=SEED)
        fresh = single(f)
    assert same(got, fresh)
    assert got[0] == orc.run_gmm(orc.config(plan, env, K=K), seed_of(0), N)["prob"]


@pytest.mark.gpu
def test_refusals(pocs, orc, plan, env):
    K, N = 3, 2000
    plans = candidates(pocs, plan, (12, 56, 5))
    with pocs.Context(0) as c:
        lib, h = c.lib, c.h
        out = (C.c_int * 8)()
        assert lib.pocs_get_plan_evaluated(h, out, 8) == -3             # before any call
        c.configure(plan, env, K=K, N=N, seed=SEED)
        c.set_plan_risk_bound(BOUND)
        c.run_gmm_estimation()                                           # a single plan: not a call of plans
        assert lib.pocs_get_plan_evaluated(h, out, 8) == -3
        c.set_plans(plans)
        assert lib.pocs_get_plan_evaluated(h, out, 8) == -3             # plans set, none evaluated yet
        for bad in (0.0, -1.0, float("nan"), -float("inf")):
            assert lib.pocs_set_plan_risk_bound(h, bad) == -1, bad
            assert "risk bound" in lib.pocs_last_error(h).decode()
        c.set_seed(SEED)
        c.run_gmm_estimation()                                           # still usable, the bound as it was
        exps = [expected(orc, pl, env, K, seed_of(p), N, BOUND) for p, pl in enumerate(plans)]
        assert exps[1]["E"] < 56
        assert lib.pocs_get_plan_evaluated(h, out, 2) == -6
        assert lib.pocs_get_plan_evaluated(h, None, 8) == -1
        assert lib.pocs_get_plan_evaluated(h, out, 3) == 3 and list(out[:3]) == [e["E"] for e in exps]
        assert c.batch_probabilities().tolist() == [e["prob"] for e in exps]


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [0, 1])
def test_mc_ignores_the_bound(ctx, pocs, orc, plan, env, fused):
    K, N = 1, 3001
    plans = candidates(pocs, plan)
    configured(ctx, pocs, plan, env, plans, K, N, BOUND)
    ctx.set_option(pocs.OPT_MC_FUSED, fused)
    try:
        ctx.run_gmm_estimation()                                         # (a stopped GMM call first)
        assert (ctx.plan_evaluated() < np.array(LENGTHS)).any()
        ctx.set_seed(SEED)
        p0 = ctx.run_simulation()
        counts, probs = ctx.mc_batch_counts(), ctx.batch_probabilities()
        assert ctx.plan_evaluated().tolist() == list(LENGTHS) and p0 == probs[0]
        for p, pl in enumerate(plans):
            n, _, _ = orc.run_mc(orc.config(pl, env, K=K), seed_of(p), N)
            assert counts[p] == n and probs[p] == n / N, p
    finally:
        ctx.set_option(pocs.OPT_MC_FUSED, 0)
        ctx.set_plan_risk_bound(1.0)
