"""Batches of candidate plans (pocs_set_plans): one call evaluates P plans of different lengths, and every plan gets
bit for bit what a context holding that plan alone computes -- which the oracle restates plan by plan.  The packing
of the plans is checked on the CPU; everything that launches is marked `gpu`."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

SEED = 0x5EED0001
WEYL = 0x9E3779B97F4A7C15            # effective seed of the r-th run of a context = seed + r * WEYL (mod 2^64)
ROOT = Path(__file__).resolve().parents[1]
LENGTHS = (20, 56, 1, 33, 2, 56, 7, 120)      # unsorted on purpose; the two 56s are different plans


def seed_of(r):
    return (SEED + r * WEYL) % 2**64


def shifted(pocs, plan, dy):
    traj = np.asarray(plan["traj"]) + np.array([0.0, dy, 0.0])
    return dict(traj=traj, odom=pocs.planio.path_odometry(traj))


def prefix(plan, W):
    return dict(traj=np.asarray(plan["traj"])[:W].copy(), odom=np.asarray(plan["odom"])[:W - 1].copy().reshape(-1, 3))


def candidates(pocs, plan, lengths=LENGTHS):
    """Plans of the given lengths made from the bundled one (W = 56): prefixes, resampled copies (other lengths) and a
    laterally shifted copy (the second 56), so that their probabilities differ."""
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


# ---- CPU -----------------------------------------------------------------------------------------------------------

def test_set_plans_is_declared_and_wrapped(pocs):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pocs.h").read_text(), flags=re.S)
    assert re.search(r"int\s+pocs_set_plans\s*\(\s*pocs_ctx\s*\*\s*ctx\s*,\s*int\s+P\s*,\s*const\s+int\s*\*\s*W\s*,"
                     r"\s*const\s+double\s*\*\s*trajs\s*,\s*const\s+double\s*\*\s*odoms\s*\)", text)
    assert re.search(r"#define\s+POCS_OPT_PLAN_SEEDS\s+10\b", (ROOT / "include" / "pocs.h").read_text())
    assert "pocs_set_plans" in pocs.SIGNATURES and pocs.OPT_PLAN_SEEDS == 10


def test_pack_plans_layout(pocs, plan):
    plans = candidates(pocs, plan, (3, 1, 5))
    W, trajs, odoms = pocs.pack_plans(plans)
    assert W.dtype == np.int32 and list(W) == [3, 1, 5]
    assert trajs.dtype == np.float64 and trajs.shape == (3 * 9,) and odoms.shape == (3 * 6,)
    to = oo = 0
    for p, pl in zip(W, plans):
        t, o = np.asarray(pl["traj"]), np.asarray(pl["odom"]).reshape(-1, 3)
        for c in range(3):                          # by component, as pocs_set_trajectory / pocs_set_odometry take one plan
            assert np.array_equal(trajs[to + c * p: to + (c + 1) * p], t[:, c])
            assert np.array_equal(odoms[oo + c * (p - 1): oo + (c + 1) * (p - 1)], o[:, c])
        to += 3 * p
        oo += 3 * (p - 1)
    assert to == trajs.size and oo == odoms.size
    # one plan alone is what set_plan sends
    W1, t1, o1 = pocs.pack_plans([plan])
    assert list(W1) == [56] and np.array_equal(t1, np.asarray(plan["traj"]).T.ravel())
    assert np.array_equal(o1, np.asarray(plan["odom"]).T.ravel())


def test_pack_plans_rejects_bad_plans(pocs, plan):
    good = prefix(plan, 5)
    with pytest.raises(ValueError):
        pocs.pack_plans([])                                                         # P = 0: clear_plans does that
    with pytest.raises(ValueError):
        pocs.pack_plans([good] * 257)                                               # P > 256
    with pytest.raises(ValueError):
        pocs.pack_plans([good, dict(traj=np.zeros((0, 3)), odom=np.zeros((0, 3)))])     # W < 1
    with pytest.raises(ValueError):
        pocs.pack_plans([dict(traj=good["traj"], odom=good["odom"][:2])])            # odometry of W - 2 steps
    with pytest.raises(ValueError):
        pocs.pack_plans([dict(traj=good["traj"][:, :2], odom=good["odom"])])         # W x 2 trajectory
    with pytest.raises(ValueError):
        pocs.pack_plans([dict(traj=good["traj"], odom=good["odom"].T)])              # odometry transposed


# ---- GPU -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx(pocs):
    c = pocs.Context(0)
    yield c
    c.close()


def configured(c, pocs, plan, env, plans, K, N, seed=SEED):
    if getattr(c, "_single_batch", None) is not None:
        c.clear_plans()
    c.configure(plan, env, K=K, N=N, seed=seed)
    c.set_plans(plans)


def plan_view(c, p, K):
    c.select_batch_run(p)
    W = c.path_length()
    return dict(W=W, probs=c.waypoint_probabilities().copy(), moments=np.array([c.moments(w, K) for w in range(W)]),
                states=np.array([c.gmm_state_raw(w, K) for w in range(W)])[..., :14])


@pytest.mark.gpu
@pytest.mark.parametrize("K,N", [(1, 3001), (3, 5000), (8, 2048)])
def test_plans_match_the_oracle(ctx, pocs, orc, plan, env, K, N):
    plans = candidates(pocs, plan)
    configured(ctx, pocs, plan, env, plans, K, N)
    p0 = ctx.run_gmm_estimation()
    finals = ctx.batch_probabilities()
    assert len(finals) == len(plans) and p0 == finals[0]
    assert len(set(finals.tolist())) > 2, finals                      # the plans are told apart
    for p, pl in enumerate(plans):
        cfg = orc.config(pl, env, K=K)
        want = orc.run_gmm(cfg, seed_of(p), N)
        got = plan_view(ctx, p, K)
        assert got["W"] == len(pl["traj"]), p
        assert finals[p] == want["prob"], p
        assert np.array_equal(got["probs"], want["probs"]), p
        assert np.array_equal(got["moments"], want["moments"]), p
        for w in sorted({0, got["W"] // 2, got["W"] - 1}):
            assert np.array_equal(got["states"][w], want["states"][w][..., :14]), (p, w)
        # past the plan's end there is nothing to get
        with pytest.raises(pocs.PocsError) as e:
            ctx.moments(got["W"], K)
        assert e.value.code == -1
        with pytest.raises(pocs.PocsError) as e:
            ctx.gmm_state(got["W"], K)
        assert e.value.code == -1
        if got["W"] > 1:
            hc, wc = ctx.host_chain(8), orc.host_chain(cfg, seed_of(p))
            for k in ("applied", "noisy", "z", "mu", "cov"):
                assert np.array_equal(hc[k], wc[k]), (p, k)
    # the last waypoint's samples of a selected plan are that plan's
    p = 3
    ctx.select_batch_run(p)
    want = orc.run_gmm(orc.config(plans[p], env, K=K), seed_of(p), N, want_samples=True)
    xyz, flags = ctx.gmm_samples(N)
    assert np.array_equal(flags, want["flags"]) and np.array_equal(xyz, want["samples"])


def _all_results(c, n, K):
    return [np.float64(x) for x in c.batch_probabilities()] + [plan_view(c, p, K)[k] for p in range(n) for k in ("probs", "moments", "states")]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
def test_launch_forms_change_no_bit(pocs, orc, plan, env):
    """Sub-batches 1 and 2, graph replay and eager launches, samples stored or not, the profiling form: the same bits.
    Then eight plans at a sample count where the default rule takes two sub-batches, against one sub-batch and the
    oracle."""
    K, N = 3, 40001
    plans = candidates(pocs, plan)
    with pocs.Context(0) as c:
        c.configure(plan, env, K=K, N=N, seed=SEED)
        c.set_plans(plans)
        outs = []
        for sub, graph, store in ((1, 1, 1), (2, 1, 1), (2, 0, 1), (1, 0, 0), (2, 1, 0), (2, 1, 1)):
            c.set_option(pocs.OPT_SUB_BATCHES, sub)
            c.set_option(pocs.OPT_USE_GRAPH, graph)
            c.set_option(pocs.OPT_STORE_SAMPLES, store)
            c.set_seed(SEED)
            c.run_gmm_estimation()
            outs.append(_all_results(c, len(plans), K))
        c.set_option(pocs.OPT_PROFILE, 1)
        c.set_seed(SEED)
        c.run_gmm_estimation()
        assert c.sequence_time()[1] == 2
        outs.append(_all_results(c, len(plans), K))
        for i, o in enumerate(outs[1:]):
            assert _same(o, outs[0]), i + 1
        want = orc.run_gmm(orc.config(plans[7], env, K=K), seed_of(7), N)
        assert outs[0][7] == want["prob"]

        N = 160000                                       # 8 plans x 1.6e5 samples: two sub-batches by default
        c.set_option(pocs.OPT_PROFILE, 0)
        c.set_option(pocs.OPT_STORE_SAMPLES, 1)
        c.set_num_gmm_samples(N)
        big = []
        for sub in (0, 1):
            c.set_option(pocs.OPT_SUB_BATCHES, sub)
            c.set_option(pocs.OPT_USE_GRAPH, 1)
            c.set_seed(SEED)
            c.run_gmm_estimation()
            big.append(_all_results(c, len(plans), K) + list(c.gmm_samples(N)))
        assert _same(big[1], big[0])
        for p in (2, 7):
            want = orc.run_gmm(orc.config(plans[p], env, K=K), seed_of(p), N)
            assert big[0][p] == want["prob"] and np.array_equal(big[0][8 + 3 * p + 1], want["moments"]), p


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [0, 1])
def test_mc_plans_match_the_oracle(ctx, pocs, orc, plan, env, fused):
    K, N = 1, 3001
    plans = candidates(pocs, plan)
    configured(ctx, pocs, plan, env, plans, K, N)
    ctx.set_option(pocs.OPT_MC_FUSED, fused)
    try:
        p0 = ctx.run_simulation()
        counts = ctx.mc_batch_counts()
        probs = ctx.batch_probabilities()
        assert len(counts) == len(plans) and p0 == probs[0]
        for p, pl in enumerate(plans):
            n, hits, parts = orc.run_mc(orc.config(pl, env, K=K), seed_of(p), N, want_particles=p in (1, 4, 7))
            assert counts[p] == n and probs[p] == n / N, p
            if parts is not None:
                ctx.select_batch_run(p)
                assert ctx.path_length() == len(pl["traj"])
                xyz, got_hits = ctx.particles(N)
                assert np.array_equal(got_hits, hits) and np.array_equal(xyz, parts), p
    finally:
        ctx.set_option(pocs.OPT_MC_FUSED, 0)


@pytest.mark.gpu
def test_common_random_numbers(ctx, pocs, orc, plan, env):
    K, N = 3, 4000
    plans = candidates(pocs, plan, (33, 56, 7, 56))
    plans.append(plans[1])                                            # two identical plans
    configured(ctx, pocs, plan, env, plans, K, N)
    ctx.set_option(pocs.OPT_PLAN_SEEDS, 1)
    try:
        first = ctx.run_gmm_estimation()
        fin = ctx.batch_probabilities()
        views = [plan_view(ctx, p, K) for p in range(len(plans))]
        for p, pl in enumerate(plans):                               # every plan on the stream of run_index (0)
            want = orc.run_gmm(orc.config(pl, env, K=K), seed_of(0), N)
            assert fin[p] == want["prob"] and np.array_equal(views[p]["moments"], want["moments"]), p
        assert fin[1] == fin[4] and all(np.array_equal(views[1][k], views[4][k]) for k in ("probs", "moments", "states"))
        # the counter advanced by one: the next call draws run 1's stream for every plan
        ctx.run_gmm_estimation()
        fin2 = ctx.batch_probabilities()
        for p in (0, 2):
            assert fin2[p] == orc.run_gmm(orc.config(plans[p], env, K=K), seed_of(1), N)["prob"], p
        # permuting the plans permutes the results
        perm = [3, 0, 4, 2, 1]
        ctx.set_plans([plans[i] for i in perm])
        ctx.set_seed(SEED)
        assert ctx.run_gmm_estimation() == fin[perm[0]]
        fp = ctx.batch_probabilities()
        for q, i in enumerate(perm):
            assert fp[q] == fin[i]
            assert np.array_equal(plan_view(ctx, q, K)["moments"], views[i]["moments"]), q
        assert first == fin[0]
    finally:
        ctx.set_option(pocs.OPT_PLAN_SEEDS, 0)
    # the default: plan p draws run p's stream, and the counter advances by P
    ctx.set_seed(SEED)
    ctx.run_gmm_estimation()
    ctx.run_gmm_estimation()
    P = len(perm)
    for q in (0, 3):
        want = orc.run_gmm(orc.config(plans[perm[q]], env, K=K), seed_of(P + q), N)
        assert ctx.batch_probabilities()[q] == want["prob"], q


@pytest.mark.gpu
@pytest.mark.parametrize("W", [56, 33])
def test_one_plan_is_the_single_call(pocs, plan, env, W):
    """P = 1 takes the lone form, as one run per call does: the same bits as the single call on that plan, and
    run-ahead does not apply (the run counter advances by one per call)."""
    K, N = 3, 30000
    pl = candidates(pocs, plan, (W,))[0]
    with pocs.Context(0) as c:
        c.configure(pl, env, K=K, N=N, seed=SEED)
        singles = []
        for _ in range(2):
            p = c.run_gmm_estimation()
            singles.append([np.float64(p)] + [plan_view(c, 0, K)[k] for k in ("probs", "moments", "states")] + list(c.gmm_samples(N)))
        c.set_plans([pl])
        c.set_option(pocs.OPT_RUN_AHEAD, 8)
        c.set_seed(SEED)
        for i in range(2):
            p = c.run_gmm_estimation()
            got = [np.float64(p)] + [plan_view(c, 0, K)[k] for k in ("probs", "moments", "states")] + list(c.gmm_samples(N))
            assert _same(got, singles[i]), i
            assert list(c.batch_probabilities()) == [p]


@pytest.mark.gpu
def test_graph_cache_and_clearing(pocs, orc, plan, env):
    K, N = 3, 6000
    A = candidates(pocs, plan, (20, 56, 7, 33))
    B = candidates(pocs, plan, (56, 10, 40, 3))                     # same P and longest plan, other lengths
    with pocs.Context(0) as c:
        c.configure(plan, env, K=K, N=N, seed=SEED)
        c.set_plans(A)
        c.run_gmm_estimation()
        c.set_plans(B)
        c.set_seed(SEED)
        c.run_gmm_estimation()
        fin = c.batch_probabilities()
        for p, pl in enumerate(B):
            want = orc.run_gmm(orc.config(pl, env, K=K), seed_of(p), N)
            assert fin[p] == want["prob"] and np.array_equal(plan_view(c, p, K)["moments"], want["moments"]), p
        c.run_simulation()                                           # (an MC call of plans in between)
        c.clear_plans()
        assert c.path_length() == 56
        c.set_seed(SEED)
        got = [np.float64(c.run_gmm_estimation())] + [plan_view(c, 0, K)[k] for k in ("probs", "moments", "states")]
        assert len(c.batch_probabilities()) == 1
    with pocs.Context(0) as f:
        f.configure(plan, env, K=K, N=N, seed=SEED)
        fresh = [np.float64(f.run_gmm_estimation())] + [plan_view(f, 0, K)[k] for k in ("probs", "moments", "states")]
    assert _same(got, fresh)


@pytest.mark.gpu
def test_refusals_leave_the_context_usable(ctx, pocs, orc, plan, env):
    K, N = 3, 2000
    plans = candidates(pocs, plan, (12, 30, 5))
    configured(ctx, pocs, plan, env, plans, K, N)
    lib, h = ctx.lib, ctx.h
    traj = np.ascontiguousarray(np.asarray(plan["traj"]).T)
    odom = np.ascontiguousarray(np.asarray(plan["odom"]).T)
    dp = C.POINTER(C.c_double)
    for rc in (lib.pocs_set_batch(h, 4), lib.pocs_set_path_length(h, 56),
               lib.pocs_set_trajectory(h, traj.ctypes.data_as(dp), 56), lib.pocs_set_odometry(h, odom.ctypes.data_as(dp), 55)):
        assert rc == -2
        assert "pocs_set_plans(ctx, 0" in lib.pocs_last_error(h).decode()
    with pytest.raises(pocs.PocsError) as e:
        ctx.send_command("setBatch 4")
    assert e.value.code == -2
    assert lib.pocs_set_shard(h, 0, 1000) == -3
    assert lib.pocs_set_shard(h, -1, -1) == 0
    assert lib.pocs_gmm_begin(h) == -3
    assert lib.pocs_xchg_create(h, 2, 0, C.create_string_buffer(64)) == -3
    # bad plans
    W, trajs, odoms = pocs.pack_plans(plans)
    ip = C.POINTER(C.c_int)
    assert lib.pocs_set_plans(h, 257, W.ctypes.data_as(ip), trajs.ctypes.data_as(dp), odoms.ctypes.data_as(dp)) == -1
    assert lib.pocs_set_plans(h, -1, W.ctypes.data_as(ip), trajs.ctypes.data_as(dp), odoms.ctypes.data_as(dp)) == -1
    assert lib.pocs_set_plans(h, 3, None, trajs.ctypes.data_as(dp), odoms.ctypes.data_as(dp)) == -1
    assert lib.pocs_set_plans(h, 3, W.ctypes.data_as(ip), None, odoms.ctypes.data_as(dp)) == -1
    assert lib.pocs_set_plans(h, 3, W.ctypes.data_as(ip), trajs.ctypes.data_as(dp), None) == -1
    W0 = W.copy()
    W0[1] = 0
    assert lib.pocs_set_plans(h, 3, W0.ctypes.data_as(ip), trajs.ctypes.data_as(dp), odoms.ctypes.data_as(dp)) == -1
    # still usable, the plans as they were
    ctx.set_seed(SEED)
    ctx.run_gmm_estimation()
    fin = ctx.batch_probabilities()
    for p, pl in enumerate(plans):
        assert fin[p] == orc.run_gmm(orc.config(pl, env, K=K), seed_of(p), N)["prob"], p
    ctx.clear_plans()
    assert lib.pocs_set_batch(h, 1) == 0
