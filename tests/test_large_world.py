"""Large collision worlds on the GPU (pocs_set_world with more than 64 boxes): both estimators against the CPU oracle's full loop
over all M boxes, and against the small-world path on worlds whose extra boxes are out of every pose's reach.

Worlds are built from the bundled plan and room (7 boxes, footprint half extents 0.334):
  clutter(M)  the room's boxes plus M - 7 random boxes with centres in x in [20, 60] -- out of every pose's reach --, the table
              shuffled with a fixed seed so that the kept records are not a prefix;
  posts       the room plus a grid of posts of half extent 0.03, spacing 0.12 over [-3.9, 3.9] x [-1.9, 1.9], yaws
              0.3 * ((i + j) mod 5), the posts within 0.5 of any nominal waypoint removed: 1435 boxes, at most 64 of them in
              reach of the run at any waypoint (asserted below on the oracle's states);
  crowd       posts plus a 10 x 10 patch of posts at spacing 0.05, centred 0.6 beside nominal waypoint 5: more than 64 in reach
              there (asserted likewise), which a GMM call refuses and an MC call does not mind.
Every expected value comes from the oracle or from the CPU harness of tests/test_large_world_host.py; every comparison is `==`."""
import numpy as np
import pytest

from test_large_world_host import harness, reach_counts
from test_mc_waypoint_counts import prefix_profile
from test_plan_risk_bound import prefix, same, shifted, view

pytestmark = pytest.mark.gpu
SEED = 4
E_ARG, E_STATE = -1, -3
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def clutter(env, M, seed=11):
    room = np.asarray(env["boxes"], np.float64).reshape(-1, 5)
    rng = np.random.default_rng(seed)
    n = M - len(room)
    far = np.column_stack([rng.uniform(20.0, 60.0, n), rng.uniform(-2.0, 2.0, n), rng.uniform(0.05, 0.4, n), rng.uniform(0.05, 0.4, n),
                           np.where(rng.random(n) < 0.3, 0.0, rng.uniform(-3.2, 3.2, n))])
    return rng.permutation(np.vstack([room, far]), axis=0)


def posts(plan, env):
    def make():
        room = np.asarray(env["boxes"], np.float64).reshape(-1, 5)
        traj = np.asarray(plan["traj"], np.float64)
        out = []
        for i in range(66):
            for j in range(32):
                x, y = -3.9 + 0.12 * i, -1.9 + 0.12 * j
                if x > 3.9 + 1e-9 or y > 1.9 + 1e-9 or np.hypot(traj[:, 0] - x, traj[:, 1] - y).min() <= 0.5:
                    continue
                out.append([x, y, 0.03, 0.03, 0.3 * ((i + j) % 5)])
        return np.vstack([room, np.array(out)])
    return cached("posts", make)


def crowd(plan, env):
    def make():
        t = np.asarray(plan["traj"], np.float64)[5]
        cx, cy = t[0] - 0.6 * np.sin(t[2]), t[1] + 0.6 * np.cos(t[2])
        patch = [[cx + 0.05 * (i - 4.5), cy + 0.05 * (j - 4.5), 0.03, 0.03, 0.3 * ((i + j) % 5)] for i in range(10) for j in range(10)]
        return np.vstack([posts(plan, env), np.array(patch)])
    return cached("crowd", make)


def world_env(env, boxes):
    return dict(footprint=env["footprint"], boxes=boxes)


def oracle_gmm(orc, pl, env, boxes, K, N, key, seed=SEED):
    return cached(("gmm", key, K, N, seed), lambda: orc.run_gmm(orc.config(pl, world_env(env, boxes), K=K), seed, N, want_samples=True))


def oracle_mc(orc, pl, env, boxes, N, key, seed=SEED):
    return cached(("mc", key, N, seed), lambda: orc.run_mc(orc.config(pl, world_env(env, boxes), K=1), seed, N, want_particles=True))


def context(pocs, pl, env, boxes, K, N, seed=SEED):
    """A context on the plan with the room's footprint and the world `boxes` through set_world."""
    c = pocs.Context(0)
    c.configure(pl, env, K=K, N=N, seed=seed)
    c.set_world(boxes)
    return c


def check_gmm(c, want, K, N):
    W = len(want["probs"])
    assert c.run_gmm_estimation() == want["prob"]
    assert np.array_equal(c.waypoint_probabilities(), want["probs"])
    for w in range(W):
        assert np.array_equal(c.moments(w, K), want["moments"][w]), w
        assert np.array_equal(c.gmm_state_raw(w, K), want["states"][w]), w
    xyz, flags = c.gmm_samples(N)
    assert np.array_equal(flags, want["flags"]) and np.array_equal(xyz, want["samples"])


def check_mc(c, want, N, seed=SEED):
    n, hits, parts = want
    c.set_seed(seed)
    assert c.run_simulation() == n / N
    assert c.mc_batch_counts() == [n]
    xyz, h = c.particles(N)
    assert np.array_equal(h, hits) and np.array_equal(xyz, parts)


def test_the_scenes_are_what_they_claim(pocs, orc, plan, env):
    lib = harness()
    fp = env["footprint"]
    assert fp[2] == fp[3] == 0.334 and len(np.asarray(env["boxes"]).reshape(-1, 5)) == 7
    p, cr = posts(plan, env), crowd(plan, env)
    assert len(p) == 1435 and len(cr) == 1535
    rp = reach_counts(lib, oracle_gmm(orc, plan, env, p, 3, 3000, "posts")["states"], fp, p)
    print("posts: boxes in reach per waypoint", rp.tolist())
    assert 40 <= rp.max() <= 64 and rp.min() >= 1
    # (the oracle's states past the overflow are the true ones -- the oracle has no cap --, the device's are not: only the
    # first waypoint above 64 is compared with the device, in test_overflow)
    rc = reach_counts(lib, oracle_gmm(orc, plan, env, cr, 3, 3000, "crowd")["states"], fp, cr)
    print("crowd: boxes in reach per waypoint", rc.tolist())
    assert rc.max() > 64
    c200 = clutter(env, 200)
    assert (reach_counts(lib, oracle_gmm(orc, plan, env, c200, 3, 1000, "c200")["states"], fp, c200) <= 7).all()


def test_65_boxes_is_the_smallest_large_world(pocs, orc, plan, env):
    K, N = 3, 3000
    boxes = clutter(env, 65)
    with context(pocs, plan, env, boxes, K, N) as c:
        assert c.world_boxes() == 65 and c.world_steps() == 1
        check_gmm(c, oracle_gmm(orc, plan, env, boxes, K, N, "c65"), K, N)
        assert (c.world_reach() <= 7).all() and len(c.world_reach()) == 56
        check_mc(c, oracle_mc(orc, plan, env, boxes, N, "c65"), N)
        with pytest.raises(pocs.PocsError) as e:                    # the old entry point keeps its limit, and the world in force stays
            c.set_env(world_env(env, boxes))
        assert e.value.code == E_ARG and c.world_boxes() == 65


@pytest.mark.parametrize("M,W,N,K", [(1024, 56, 2000, 3), (4096, 8, 1000, 3), (200, 56, 1000, 1), (200, 56, 1000, 3), (200, 56, 1000, 8)])
def test_sizes_and_numbers_of_gaussians(pocs, orc, plan, env, M, W, N, K):
    pl = prefix(plan, W)
    boxes = clutter(env, M)
    with context(pocs, pl, env, boxes, K, N) as c:
        assert c.world_boxes() == M
        check_gmm(c, oracle_gmm(orc, pl, env, boxes, K, N, ("c", M, W)), K, N)
        check_mc(c, oracle_mc(orc, pl, env, boxes, N, ("c", M, W)), N)


@pytest.mark.parametrize("N", [1, 63, 64, 65, 3001])
def test_mc_partial_and_multiple_waves(pocs, orc, plan, env, N):
    pl = prefix(plan, 12)
    boxes = posts(plan, env)
    wenv = world_env(env, boxes)
    n, hits, parts = oracle_mc(orc, pl, env, boxes, N, "posts12")
    F, _ = prefix_profile(orc, pl, wenv, SEED, N, key=("posts12", N))
    with context(pocs, pl, env, boxes, 1, N) as c:
        seen = []
        for wp in (0, 1):
            for nt in (0, 1):
                c.set_option(pocs.OPT_MC_WAYPOINT_COUNTS, wp)
                c.set_option(pocs.OPT_MC_NONTEMPORAL, nt)
                c.set_seed(SEED)
                assert c.run_simulation() == n / N and c.mc_batch_counts() == [n]
                xyz, h = c.particles(N)
                assert np.array_equal(h, hits) and np.array_equal(xyz, parts)
                if wp:
                    assert np.array_equal(c.mc_waypoint_counts(), F)
                seen.append((xyz, h))
        assert all(np.array_equal(s[0], seen[0][0]) and np.array_equal(s[1], seen[0][1]) for s in seen)


def test_dense_world(pocs, orc, plan, env):
    K, N = 3, 3000
    boxes = posts(plan, env)
    want = oracle_gmm(orc, plan, env, boxes, K, N, "posts")
    with context(pocs, plan, env, boxes, K, N) as c:
        check_gmm(c, want, K, N)
        assert np.array_equal(c.world_reach(), reach_counts(harness(), want["states"], env["footprint"], boxes))
        check_mc(c, oracle_mc(orc, plan, env, boxes, N, "posts"), N)


def gmm_batch_view(c, R, K, N):
    out = [c.batch_probabilities().copy()]
    for r in range(R):
        c.select_batch_run(r)
        W = c.path_length()
        out += [c.waypoint_probabilities().copy()] + [c.moments(w, K) for w in range(W)] + [c.gmm_state_raw(w, K) for w in (0, W // 2, W - 1)]
        out += list(c.gmm_samples(N))
    return out


def gmm_single_view(c, K, N):
    W = c.path_length()
    return [c.waypoint_probabilities().copy()] + [c.moments(w, K) for w in range(W)] + [c.gmm_state_raw(w, K) for w in range(W)] + list(c.gmm_samples(N))


def plans_view(c, n, K, N):
    out = [c.plan_evaluated().copy(), c.batch_probabilities().copy()]
    for p in range(n):
        v = view(c, p, K)
        out += [v["probs"], v["moments"]] + [v["states"][w] for w in sorted(v["states"])] + list(c.gmm_samples(N))
    return out


def mc_plans_view(c, pocs, n, N):
    out = [np.array(c.mc_batch_counts()), c.batch_probabilities().copy(), c.plan_evaluated().copy()]
    for p in range(n):
        c.select_batch_run(p)
        out += [c.mc_waypoint_counts().copy()] + list(c.particles(N))
    return out


def both(pocs, plan, env, K, N, body):
    """body(context) on the room through set_env and on clutter(200) through set_world: the two results."""
    got = []
    for large in (False, True):
        with pocs.Context(0) as c:
            c.configure(plan, env, K=K, N=N, seed=SEED)
            if large:
                c.set_world(clutter(env, 200))
            got.append(body(c, large))
    return got


def test_differential_batches_and_run_ahead(pocs, plan, env):
    K = 3

    def batch5(c, large):
        c.set_batch(5)
        p = c.run_gmm_estimation()
        g = [p] + gmm_batch_view(c, 5, K, 2000)
        c.set_seed(SEED)
        return g + [c.run_simulation(), np.array(c.mc_batch_counts())]
    a, b = both(pocs, plan, env, K, 2000, batch5)
    assert same(a, b)

    def run_ahead(c, large):
        c.set_option(pocs.OPT_RUN_AHEAD, 8)
        out = []
        for r in range(9):                  # eight served from one launch, the ninth from the next
            out += [c.run_gmm_estimation()] + gmm_single_view(c, K, 1500)[:8]
            if large:
                assert len(c.world_reach()) == 56 and (c.world_reach() <= 7).all()
        return out
    a, b = both(pocs, plan, env, K, 1500, run_ahead)
    assert same(a, b)

    def batch20(c, large):                  # 20 x 70000 evaluations per waypoint: two sub-batches on two streams
        c.set_batch(20)
        c.set_option(pocs.OPT_STORE_SAMPLES, 0)
        out = [c.run_gmm_estimation(), c.batch_probabilities().copy()]
        for r in (0, 9, 10, 19):
            c.select_batch_run(r)
            out += [c.waypoint_probabilities().copy()] + [c.moments(w, K) for w in range(56)] + [c.gmm_state_raw(w, K) for w in (0, 30, 55)]
        return out
    a, b = both(pocs, plan, env, K, 70000, batch20)
    assert same(a, b)


def test_differential_plans_and_the_risk_bound(pocs, plan, env):
    K, N = 3, 3000
    plans = [plan, prefix(plan, 30), prefix(plan, 9)]

    def body(c, large):
        out = []
        c.set_plans(plans)
        for bound in (1.0, 0.2):
            c.set_plan_risk_bound(bound)
            c.set_seed(SEED)
            out += [c.run_gmm_estimation()] + plans_view(c, 3, K, N)
            if large:
                for p in range(3):
                    c.select_batch_run(p)
                    r, E = c.world_reach(), int(c.plan_evaluated()[p])
                    assert len(r) == len(plans[p]["traj"]) and r[0] >= 1 and r[:E].max() <= 7 and (r[E:] == 0).all(), (bound, p, r, E)
        stopped = c.plan_evaluated().copy()
        c.set_option(pocs.OPT_MC_RISK_BOUND, 1)
        c.set_seed(SEED)
        out += [c.run_simulation()] + mc_plans_view(c, pocs, 3, N)
        return out + [stopped]
    a, b = both(pocs, plan, env, K, N, body)
    assert same(a, b)
    assert (a[-1] < [56, 30, 9]).any()                              # the bound stops something


def test_differential_stopped_next_to_live_runs_in_one_block(pocs, plan, env):
    """tests/test_plan_risk_bound.py's five plans of 262144 samples -- a block's range crosses from a stopped run into a live one
    and the other way round --, whose heads under a large world fetch the live run's records into the right buffer."""
    K, N = 3, 262144
    up = shifted(pocs, plan, 0.05)
    plans = [shifted(pocs, plan, -0.05), up, plan, prefix(up, 48), prefix(plan, 44)]

    def body(c, large):
        c.set_option(pocs.OPT_STORE_SAMPLES, 0)
        c.set_plans(plans)
        c.set_plan_risk_bound(0.2)
        out = [c.run_gmm_estimation(), c.plan_evaluated().copy(), c.batch_probabilities().copy()]
        for p in range(5):
            v = view(c, p, K)
            out += [v["probs"], v["moments"]]
        return out
    a, b = both(pocs, plan, env, K, N, body)
    assert same(a, b)
    E = a[1]
    assert (E < [56, 56, 56, 48, 44]).any() and (E == [56, 56, 56, 48, 44]).any()


def test_lone_call_option_changes_no_bit(pocs, plan, env):
    K, N = 3, 3000
    got = []
    for lone in (1, 0):
        with context(pocs, plan, env, clutter(env, 200), K, N) as c:
            c.set_option(pocs.OPT_LONE_CALL, lone)
            got.append([c.run_gmm_estimation()] + gmm_single_view(c, K, N) + [c.world_reach().copy()])
    assert same(got[0], got[1])
    with pocs.Context(0) as c:                                      # ... and both equal the small world's lone form
        c.configure(plan, env, K=K, N=N, seed=SEED)
        assert same(got[0][:-1], [c.run_gmm_estimation()] + gmm_single_view(c, K, N))


@pytest.mark.parametrize("M", [7, 64])
def test_set_world_up_to_64_boxes_is_set_obstacles(pocs, plan, env, M):
    K, N = 3, 2000
    boxes = clutter(env, M) if M > 7 else np.asarray(env["boxes"], np.float64).reshape(-1, 5)
    got = []
    for through_world in (False, True):
        with pocs.Context(0) as c:
            c.configure(plan, env, K=K, N=N, seed=SEED)
            assert c.world_boxes() == 7 and c.world_steps() == 1
            if through_world:
                c.set_world(boxes)
            else:
                c.set_env(world_env(env, boxes))
            assert c.world_boxes() == M and c.world_steps() == 1
            out = [c.run_gmm_estimation()] + gmm_single_view(c, K, N)
            if through_world:
                with pytest.raises(pocs.PocsError) as e:            # no cull launch, nothing to report
                    c.world_reach()
                assert e.value.code == E_STATE
            c.set_seed(SEED)
            out += [c.run_simulation()] + list(c.particles(N))
            got.append(out)
    assert same(got[0], got[1])
    with pocs.Context(0) as c:
        assert c.world_boxes() == 0 and c.world_steps() == 0
        c.set_obstacle_schedule(np.stack([boxes, boxes]))
        assert c.world_boxes() == M and c.world_steps() == 2


def test_replacing_the_world(pocs, orc, plan, env):
    """set_world, set_env, set_world with other numbers at the same M: each call sees its own world (the graphs' epoch)."""
    K, N = 3, 1000
    A = clutter(env, 100)
    B = A.copy()
    B[B[:, 0] < 10.0, 1] += 0.07                                    # the room's boxes, moved
    room = np.asarray(env["boxes"], np.float64).reshape(-1, 5)
    wa, wr, wb = (oracle_gmm(orc, plan, env, b, K, N, k) for b, k in ((A, "A"), (room, "room"), (B, "B")))
    assert wa["prob"] != wb["prob"]
    with pocs.Context(0) as c:
        c.configure(plan, env, K=K, N=N, seed=SEED)
        for setter, boxes, want, M in ((c.set_world, A, wa, 100), (None, room, wr, 7), (c.set_world, B, wb, 100), (c.set_world, A, wa, 100)):
            if setter:
                setter(boxes)
            else:
                c.set_env(env)
            assert c.world_boxes() == M
            c.set_seed(SEED)
            check_gmm(c, want, K, N)
            c.set_seed(SEED)
            assert c.run_simulation() == oracle_mc(orc, plan, env, boxes, N, ("repl", M, float(boxes[:, 1].sum())))[0] / N


def test_a_new_footprint_re_prepares_the_large_world(pocs, orc, plan, env):
    K, N = 3, 1000
    boxes = clutter(env, 100)
    env2 = dict(footprint=[0.05, 0.0, 0.4, 0.25], boxes=None)
    with context(pocs, plan, env, boxes, K, N) as c:
        c.run_gmm_estimation()
        c.set_env(env2)                                             # footprint only: the world stays
        assert c.world_boxes() == 100
        c.set_seed(SEED)
        check_gmm(c, orc.run_gmm(orc.config(plan, dict(footprint=env2["footprint"], boxes=boxes), K=K), SEED, N, want_samples=True), K, N)
        c.set_seed(SEED)
        assert c.run_simulation() == orc.run_mc(orc.config(plan, dict(footprint=env2["footprint"], boxes=boxes), K=K), SEED, N)[0] / N


def test_overflow(pocs, orc, plan, env):
    K, N = 3, 3000
    cr, p = crowd(plan, env), posts(plan, env)
    rc = reach_counts(harness(), oracle_gmm(orc, plan, env, cr, K, N, "crowd")["states"], env["footprint"], cr)
    w0 = int(np.nonzero(rc > 64)[0][0])
    with context(pocs, plan, env, cr, K, N) as c:
        with pytest.raises(pocs.PocsError) as e:
            c.run_gmm_estimation()
        assert e.value.code == E_STATE and "waypoint %d," % w0 in str(e.value) and "%d boxes" % rc[w0] in str(e.value), str(e.value)
        got = c.world_reach()
        assert len(got) == 56 and np.array_equal(got[:w0 + 1], rc[:w0 + 1]) and got[w0] > 64
        assert len(c.waypoint_probabilities()) == 0                 # the results are gone
        check_mc(c, oracle_mc(orc, plan, env, cr, N, "crowd"), N)   # MC has no cap
        c.set_world(p)                                              # the same context goes on
        c.set_seed(SEED)
        check_gmm(c, oracle_gmm(orc, plan, env, p, K, N, "posts"), K, N)


def test_refusals(pocs, orc, plan, env):
    K, N = 3, 1000
    boxes = clutter(env, 100)
    want = oracle_gmm(orc, plan, env, boxes, K, N, "c100")
    with context(pocs, plan, env, boxes, K, N) as c:
        def refused(call, codes=(E_STATE,)):
            with pytest.raises(pocs.PocsError) as e:
                call()
            assert e.value.code in codes and ("world" in str(e.value)), str(e.value)
            assert c.world_boxes() == 100
        refused(lambda: c.set_option(pocs.OPT_OBSTACLE_COUNTS, 1))
        refused(lambda: c.set_option(pocs.OPT_MC_FUSED, 1))
        refused(lambda: c.set_plan_tree([-1, 0], np.zeros((2, 3)), np.zeros((2, 3))))
        refused(lambda: c.set_shard(0, 500))
        refused(lambda: c.gmm_begin())
        refused(lambda: c.xchg_create(1, 0))
        refused(lambda: c.probe_device_collide(np.zeros((1, 12)), np.zeros((2, 3))))
        refused(lambda: c.send_command("addObstacle 0 0 1 1 0"), (E_ARG,))
        with pytest.raises(pocs.PocsError) as e:                    # schedules keep their limit
            c.set_obstacle_schedule(boxes[None, :65])
        assert e.value.code == E_ARG and c.world_boxes() == 100
        # bad tables: the world in force stays
        big = clutter(env, 4097)
        for bad in (big, np.where(np.arange(500)[:, None] * 5 + np.arange(5) == 1502, np.nan, clutter(env, 500)),
                    np.where(np.arange(500)[:, None] * 5 + np.arange(5) == 1503, 0.0, clutter(env, 500))):
            with pytest.raises(pocs.PocsError) as e:
                c.set_world(bad)
            assert e.value.code == E_ARG and c.world_boxes() == 100
        assert c.lib.pocs_set_world(c.h, None, 100) == E_ARG and c.world_boxes() == 100
        c.set_seed(SEED)
        check_gmm(c, want, K, N)                                    # the context's next plain run is unchanged
    # the other order: the option first, then the large world
    for opt in (pocs.OPT_OBSTACLE_COUNTS, pocs.OPT_MC_FUSED):
        with pocs.Context(0) as c:
            c.configure(plan, env, K=K, N=N, seed=SEED)
            c.set_option(opt, 1)
            with pytest.raises(pocs.PocsError) as e:
                c.set_world(boxes)
            assert e.value.code == E_STATE and c.world_boxes() == 7
            c.set_world(boxes[:64])                                 # up to 64 boxes it is set_obstacles: served
            assert c.world_boxes() == 64
