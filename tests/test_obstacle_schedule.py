"""Moving obstacles (pocs_set_obstacle_schedule): world s is the collision world at waypoint s, the last world holds behind it.
The reference computation is COMPOSED here from the oracle as it is: the oracle exposes the GMM estimator one waypoint at a
time and takes the collision world as a field of the configuration handed to each call, and neither its host chain nor its
mixture advance reads the boxes -- so "waypoint w sees world w" is one oracle configuration per waypoint.  For MC the cloud at
waypoint w is what the oracle's roll-out of the plan's first w + 1 waypoints returns (streams are keyed by (seed, index,
waypoint), the host chain by (seed, step)), and a particle's flag at w is the oracle's predicate against world w.  Every
comparison is `==`.  The ABI and the numpy helper are checked on the CPU; everything that launches is marked `gpu`."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

SEED = 0x5EED0001
WEYL = 0x9E3779B97F4A7C15            # effective seed of the r-th run of a context = seed + r * WEYL (mod 2^64)
ROOT = Path(__file__).resolve().parents[1]
NEW = ("pocs_set_obstacle_schedule", "pocs_get_world_steps")
K, N_GMM, N_MC, W_SCENE = 2, 4096, 2048, 9
OFF = [0.9, 0.60, 0.55, 0.52, 0.50, 0.53, 0.58]
OFF_MORE = [0.51, 0.49, 0.62, 0.70, 0.80]            # worlds 7 .. 11 of the longer schedules (S = 9, S = 12)


def seed_of(r):
    return (SEED + r * WEYL) % 2**64


def prefix(plan, W):
    return dict(traj=np.asarray(plan["traj"])[:W].copy(), odom=np.asarray(plan["odom"])[:W - 1].copy().reshape(-1, 3))


def branch(pocs, plan, j, dy):
    """A copy of `plan` whose waypoints AFTER waypoint j are shifted laterally by dy, with fresh odometry from step j on;
    everything up to waypoint j -- poses and controls -- keeps its bits."""
    t, o = np.asarray(plan["traj"]).copy(), np.asarray(plan["odom"]).copy().reshape(-1, 3)
    if dy != 0.0:
        t[j + 1:, 1] += dy
        o[j:] = pocs.planio.path_odometry(t[j:])
    return dict(traj=t, odom=o)


def schedule(plan, env, S=7, shift=0.0):
    """World s: the first three boxes of the bundled world and one moving box of half extents 0.15 x 0.15 and yaw 0.1 s, centred
    `off[s]` beside waypoint min(s + 1, 8) of the plan."""
    base = np.asarray(env["boxes"], dtype=np.float64).reshape(-1, 5)[:3]
    traj = np.asarray(plan["traj"])
    off = (OFF + OFF_MORE)[:S]
    out = np.zeros((S, 4, 5))
    for s in range(S):
        j = min(s + 1, 8)
        out[s, :3] = base
        out[s, 3] = [traj[j, 0], traj[j, 1] + off[s] + shift, 0.15, 0.15, 0.1 * s]
    return out


def world(sched, w):
    return sched[min(w, len(sched) - 1)]


@pytest.fixture(scope="module")
def scene(plan, env):
    return dict(plan=prefix(plan, W_SCENE), fp=list(env["footprint"]), sched=schedule(plan, env))


# ---- the composed reference, computed once per argument set and left unchanged ------------------------------------------------

_gmm_cache, _mc_cache = {}, {}


def composed_gmm(orc, plan, fp, sched, seed, N, Kc=K):
    key = (np.asarray(plan["traj"]).tobytes(), np.asarray(plan["odom"]).tobytes(), tuple(fp), sched.tobytes(), seed, N, Kc)
    if key in _gmm_cache:
        return _gmm_cache[key]
    W = len(plan["traj"])
    cfg = [orc.config(plan, dict(footprint=fp, boxes=world(sched, w)), Kc) for w in range(W)]
    chain = orc.host_chain(cfg[0], seed)
    state = orc.gmm_advance(cfg[0], orc.gmm_initial_state(cfg[0]), None)
    probs, moments, states, run = np.zeros(W), np.zeros((W, Kc, 11)), np.zeros((W, Kc, 16)), np.zeros(W)
    prod = 1.0
    for w in range(W):
        states[w] = state
        mom = orc.gmm_waypoint(cfg[w], seed, w, state, 0, N)
        moments[w] = mom
        collided = 0.0
        for k in range(Kc):                              # the columns added in component order
            collided += mom[k, 1]
        probs[w] = collided / (1.0 * float(N))
        prod *= 1.0 - probs[w]
        run[w] = 1.0 - prod
        if w + 1 < W:
            state = orc.gmm_advance(cfg[w], state, mom, chain["applied"][w], chain["Mdiag"][w], chain["z"][w])
    out = dict(prob=1.0 - prod, probs=probs, moments=moments, states=states[..., :14], running=run)
    _gmm_cache[key] = out
    return out


def composed_mc(orc, plan, fp, sched, seed, N, first=0, count=None):
    count = N if count is None else count
    key = (np.asarray(plan["traj"]).tobytes(), np.asarray(plan["odom"]).tobytes(), tuple(fp), sched.tobytes(), seed, N, first, count)
    if key in _mc_cache:
        return _mc_cache[key]
    W = len(plan["traj"])
    flags = np.zeros((W, count), dtype=bool)
    parts = None
    for w in range(W):
        cfg = orc.config(prefix(plan, w + 1), dict(footprint=fp, boxes=world(sched, 0)), K)
        _, _, parts = orc.run_mc(cfg, seed, N, first, count, want_particles=True)
        boxes = world(sched, w)
        flags[w] = [orc.collides(p[0], p[1], p[2], fp, boxes) for p in parts]
    hits = flags.sum(axis=0).astype(np.uint32)
    before = np.zeros(count, dtype=bool)
    profile = np.zeros(W, dtype=np.uint64)
    for w in range(W):
        profile[w] = np.count_nonzero(flags[w] & ~before)
        before |= flags[w]
    out = dict(xyz=parts, hits=hits, profile=profile, collided=int(np.count_nonzero(hits)))
    _mc_cache[key] = out
    return out


def mc_stop(profile, N, bound):
    """The rule of include/pocs.h: the first waypoint s with (double)C[s] / (double)N >= bound; a stop at the last waypoint
    stops nothing.  -> (waypoints evaluated, collided particles reported)."""
    C_s = 0
    for s in range(len(profile) - 1):
        C_s += int(profile[s])
        if float(C_s) / float(N) >= bound:
            return s + 1, C_s
    return len(profile), int(profile.sum())


# ---- CPU --------------------------------------------------------------------------------------------------------------------

def test_schedule_abi_is_declared_exported_and_wrapped(pocs):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pocs.h").read_text(), flags=re.S)
    assert re.search(r"int\s+pocs_set_obstacle_schedule\s*\(\s*pocs_ctx\s*\*\s*ctx\s*,\s*const\s+double\s*\*\s*boxes\s*,\s*int\s+M\s*,"
                     r"\s*int\s+S\s*\)", text)
    assert re.search(r"int\s+pocs_get_world_steps\s*\(\s*const\s+pocs_ctx\s*\*\s*ctx\s*\)", text)
    assert re.search(r"#define\s+POCS_MAX_WORLD_STEPS\s+4096\b", text)
    for name in NEW:
        assert name in pocs.SIGNATURES, name
    for meth in ("set_obstacle_schedule", "world_steps"):
        assert callable(getattr(pocs.Context, meth)), meth
    lib = pocs.load_library()
    for name in NEW:
        assert hasattr(lib, name), "libpocs.so does not export %s" % name


def test_moving_boxes_is_its_formula(pocs):
    rng = np.random.default_rng(3)
    b0 = rng.normal(size=(5, 5))
    b0[:, 2:4] = np.abs(b0[:, 2:4]) + 0.1
    vel = rng.normal(size=(5, 3)) * 0.1
    S = 11
    got = pocs.moving_boxes(b0, vel, S)
    assert got.shape == (S, 5, 5) and got.dtype == np.float64
    for s in range(S):
        for m in range(5):
            cx, cy, hx, hy, yaw = (float(v) for v in b0[m])
            vx, vy, om = (float(v) for v in vel[m])
            assert got[s, m].tolist() == [cx + s * vx, cy + s * vy, hx, hy, yaw + s * om], (s, m)
    with pytest.raises(ValueError):
        pocs.moving_boxes(b0, vel[:4], S)
    with pytest.raises(ValueError):
        pocs.moving_boxes(b0, vel, 0)


def test_moving_boxes_at_rest_repeat_the_first_world(pocs, env):
    b0 = np.asarray(env["boxes"], dtype=np.float64).reshape(-1, 5)
    got = pocs.moving_boxes(b0, np.zeros((len(b0), 3)), 6)
    assert got.shape == (6, len(b0), 5)
    for s in range(6):
        assert np.array_equal(got[s], b0)
    assert pocs.moving_boxes(np.zeros((0, 5)), np.zeros((0, 3)), 3).shape == (3, 0, 5)


# ---- GPU --------------------------------------------------------------------------------------------------------------------

def context(pocs, sc, N, sched="scene", plan=None, Kc=K, seed=SEED, fp=None):
    c = pocs.Context(0)
    c.configure(sc["plan"] if plan is None else plan, dict(footprint=sc["fp"] if fp is None else fp, boxes=sc["sched"][0]),
                K=Kc, N=N, seed=seed)
    if sched is not None:
        c.set_obstacle_schedule(sc["sched"] if isinstance(sched, str) else sched)
    return c


def gmm_view(c, Kc=K):
    W = c.path_length()
    return dict(W=W, probs=c.waypoint_probabilities().copy(), moments=np.array([c.moments(w, Kc) for w in range(W)]),
                states=np.array([c.gmm_state_raw(w, Kc) for w in range(W)])[..., :14])


def same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def is_composed(view, p, want):
    return (p == want["prob"] and np.array_equal(view["probs"], want["probs"]) and np.array_equal(view["moments"], want["moments"])
            and np.array_equal(view["states"], want["states"]))


def mc_view(c, n):
    xyz, hits = c.particles(n)
    return dict(xyz=xyz, hits=hits, wp=c.mc_waypoint_counts().copy(), counts=np.array(c.mc_batch_counts(), dtype=np.uint64))


def mc_is_composed(view, want):
    return (np.array_equal(view["xyz"], want["xyz"]) and np.array_equal(view["hits"], want["hits"])
            and np.array_equal(view["wp"], want["profile"]) and int(view["counts"][0]) == want["collided"])


@pytest.mark.gpu
@pytest.mark.parametrize("lone,N", [(1, N_GMM), (0, N_GMM), (1, 3001)])
def test_gmm_single_run_is_the_composition(pocs, orc, scene, lone, N):
    want = composed_gmm(orc, scene["plan"], scene["fp"], scene["sched"], SEED, N)
    print("composed per-waypoint probabilities:", want["probs"].tolist(), "final:", want["prob"])
    if N == N_GMM:                                       # the scene tells a schedule from both static extremes
        assert np.count_nonzero((want["probs"] > 0) & (want["probs"] < 1)) >= 3
        for s in (0, 6):
            static = orc.run_gmm(orc.config(scene["plan"], dict(footprint=scene["fp"], boxes=scene["sched"][s]), K), SEED, N)
            assert static["prob"] != want["prob"] and not np.array_equal(static["probs"], want["probs"])
    with context(pocs, scene, N) as c:
        assert c.world_steps() == 7
        c.set_option(pocs.OPT_LONE_CALL, lone)
        p = c.run_gmm_estimation()
        v = gmm_view(c)
        print("device per-waypoint probabilities:  ", v["probs"].tolist(), "final:", p)
        assert v["W"] == W_SCENE and is_composed(v, p, want)


@pytest.mark.gpu
def test_gmm_launch_shapes_equal_the_single_run(pocs, orc, scene):
    N = N_GMM
    single = []
    with context(pocs, scene, N) as c:
        for r in range(4):
            p = c.run_gmm_estimation()
            single.append((p, gmm_view(c)))
    for r in range(3):
        assert is_composed(single[r][1], single[r][0], composed_gmm(orc, scene["plan"], scene["fp"], scene["sched"], seed_of(r), N)), r
    with context(pocs, scene, N) as c:                   # a batch of 3
        c.set_batch(3)
        p0 = c.run_gmm_estimation()
        finals = c.batch_probabilities().copy()
        assert p0 == finals[0]
        for r in range(3):
            c.select_batch_run(r)
            assert finals[r] == single[r][0] and same(gmm_view(c), single[r][1]), r
    with context(pocs, scene, N) as c:                   # run-ahead 4, served over 4 calls
        c.set_option(pocs.OPT_RUN_AHEAD, 4)
        for r in range(4):
            p = c.run_gmm_estimation()
            assert p == single[r][0] and same(gmm_view(c), single[r][1]), r
    with context(pocs, scene, N) as c:                   # the step API on an unsharded context
        c.gmm_begin()
        for w in range(W_SCENE):
            c.gmm_step_local(w)
        p = c.gmm_end()
        assert p == single[0][0] and same(gmm_view(c), single[0][1])


def run_both(c, pocs, N):
    """One GMM call and one MC call per launch form, every run from the context's first seed."""
    c.set_option(pocs.OPT_MC_WAYPOINT_COUNTS, 1)
    c.set_seed(SEED)
    out = dict(p=c.run_gmm_estimation())
    out["gmm"] = gmm_view(c)
    for fused in (0, 1):
        c.set_option(pocs.OPT_MC_FUSED, fused)
        c.set_seed(SEED)
        out["pmc%d" % fused] = c.run_simulation()
        out["mc%d" % fused] = mc_view(c, N)
    return out


def same_runs(a, b):
    return a.keys() == b.keys() and all(same(a[k], b[k]) if isinstance(a[k], dict) else a[k] == b[k] for k in a)


@pytest.mark.gpu
def test_schedule_edges(pocs, orc, scene, plan, env):
    N = N_MC
    s12 = schedule(plan, env, 12)
    with context(pocs, scene, N, sched=scene["sched"][:1]) as a, context(pocs, scene, N, sched=None) as b:      # S = 1 is the static world
        assert a.world_steps() == 1 and b.world_steps() == 1
        ra, rb = run_both(a, pocs, N), run_both(b, pocs, N)
        assert same_runs(ra, rb)
        static0 = rb
    with context(pocs, scene, N, sched=s12[:9]) as c9, context(pocs, scene, N, sched=s12) as c12:            # S = W and S > W
        assert c9.world_steps() == 9 and c12.world_steps() == 12
        r9, r12 = run_both(c9, pocs, N), run_both(c12, pocs, N)
        assert is_composed(r9["gmm"], r9["p"], composed_gmm(orc, scene["plan"], scene["fp"], s12[:9], SEED, N))
        want = composed_mc(orc, scene["plan"], scene["fp"], s12[:9], SEED, N)
        assert mc_is_composed(r9["mc0"], want) and mc_is_composed(r9["mc1"], want)
        assert same_runs(r12, r9)                         # the extra worlds are never read
    with context(pocs, scene, N) as c:                    # S = 7 < W is the scene; a static world replaces the schedule
        r7 = run_both(c, pocs, N)
        assert not same(r7["gmm"], r9["gmm"]) and not same(r7["gmm"], static0["gmm"])
        b = np.ascontiguousarray(scene["sched"][0])
        c._chk(c.lib.pocs_set_obstacles(c.h, b.ctypes.data_as(C.POINTER(C.c_double)), b.shape[0]))
        assert c.world_steps() == 1
        assert same_runs(run_both(c, pocs, N), static0)
    fp2 = [0.02, -0.01, 0.30, 0.25]
    with context(pocs, scene, N) as a, context(pocs, scene, N, sched=None, fp=fp2) as b:      # the footprint behind the schedule ...
        a.set_env(dict(footprint=fp2, boxes=None))
        b.set_obstacle_schedule(scene["sched"])                                            # ... and in front of it
        ra, rb = run_both(a, pocs, N), run_both(b, pocs, N)
        assert same_runs(ra, rb)
        assert is_composed(ra["gmm"], ra["p"], composed_gmm(orc, scene["plan"], fp2, scene["sched"], SEED, N))
        assert mc_is_composed(ra["mc1"], composed_mc(orc, scene["plan"], fp2, scene["sched"], SEED, N))
    with pocs.Context(0) as c:
        assert c.world_steps() == 0
        c.set_obstacle_schedule(np.zeros((0, 0, 5)))      # S = 0 with M = 0: an explicitly empty world
        assert c.world_steps() == 1


@pytest.mark.gpu
def test_text_commands_replace_the_schedule(pocs, scene):
    """addObstacle under a schedule: world 0 plus the new box, static; clearObstacles: an empty static world."""
    N = N_MC
    box = scene["sched"][3, 3]                            # the moving box where it does the most harm
    with context(pocs, scene, N) as c, context(pocs, scene, N, sched=None) as ref:
        scheduled = run_both(c, pocs, N)
        c.send_command("addObstacle " + " ".join("%.17g" % v for v in box))
        assert c.world_steps() == 1
        ref.set_env(dict(footprint=scene["fp"], boxes=np.vstack([scene["sched"][0], box[None]])))
        got, want = run_both(c, pocs, N), run_both(ref, pocs, N)
        assert same_runs(got, want) and not same_runs(got, scheduled)
        c.set_obstacle_schedule(scene["sched"])
        assert c.world_steps() == 7 and same_runs(run_both(c, pocs, N), scheduled)
        c.send_command("clearObstacles")
        assert c.world_steps() == 1
        ref.set_env(dict(footprint=scene["fp"], boxes=np.zeros((0, 5))))
        got = run_both(c, pocs, N)
        assert same_runs(got, run_both(ref, pocs, N)) and got["p"] == 0.0 and got["pmc1"] == 0.0


@pytest.mark.gpu
def test_no_stale_world_after_a_new_schedule(pocs, scene, plan, env):
    """The captured graphs bake the records' addresses in: a schedule that grows moves the table, one of the same size with other
    numbers overwrites it.  Both must be seen by the next call (POCS_OPT_USE_GRAPH at its default)."""
    N = N_MC
    A, B, Cc = scene["sched"][:2], scene["sched"], schedule(plan, env, 7, shift=-0.04)
    got = []
    with context(pocs, scene, N, sched=A) as c:
        for s in (A, B, Cc):
            c.set_obstacle_schedule(s)
            assert c.world_steps() == len(s)
            got.append(run_both(c, pocs, N))
            got.append(run_both(c, pocs, N))              # (and once more, replayed)
    want = []
    for s in (A, B, Cc):
        with context(pocs, scene, N, sched=s) as c:
            want.append(run_both(c, pocs, N))
    for i in range(3):
        assert same_runs(got[2 * i], want[i]) and same_runs(got[2 * i + 1], want[i]), i
    assert not same_runs(want[0], want[1]) and not same_runs(want[1], want[2])


@pytest.mark.gpu
@pytest.mark.parametrize("N", [100, N_MC, 2500])
def test_mc_is_the_composition_in_both_launch_forms(pocs, orc, scene, N):
    want = composed_mc(orc, scene["plan"], scene["fp"], scene["sched"], SEED, N)
    print("composed first-collision profile:", want["profile"].tolist(), "collided:", want["collided"])
    if N == N_MC:
        assert np.count_nonzero(want["profile"]) >= 3
        for s in (0, 6):
            static = composed_mc(orc, scene["plan"], scene["fp"], scene["sched"][s:s + 1], SEED, N)
            assert not np.array_equal(static["profile"], want["profile"])
    n_full, _, full = orc.run_mc(orc.config(scene["plan"], dict(footprint=scene["fp"], boxes=scene["sched"][0]), K), SEED, N, want_particles=True)
    assert np.array_equal(full, want["xyz"])              # the cloud of the full plan
    views = []
    with context(pocs, scene, N) as c:
        c.set_option(pocs.OPT_MC_WAYPOINT_COUNTS, 1)
        for fused in (0, 1):
            c.set_option(pocs.OPT_MC_FUSED, fused)
            c.set_seed(SEED)
            p = c.run_simulation()
            v = mc_view(c, N)
            print("device profile (fused %d):        " % fused, v["wp"].tolist(), "collided:", int(v["counts"][0]))
            assert p == want["collided"] / N and mc_is_composed(v, want), fused
            views.append(v)
        assert same(views[0], views[1])
        if N == N_MC:                                     # a batch of 3 in the fused form, run by run
            c.set_batch(3)
            c.set_seed(SEED)
            c.run_simulation()
            counts = c.mc_batch_counts()
            for r in range(3):
                c.select_batch_run(r)
                xyz, hits = c.particles(N)
                w = composed_mc(orc, scene["plan"], scene["fp"], scene["sched"], seed_of(r), N)
                assert counts[r] == w["collided"] and np.array_equal(xyz, w["xyz"]) and np.array_equal(hits, w["hits"]), r
                assert np.array_equal(c.mc_waypoint_counts(), w["profile"]), r
        if N == 2500:                                     # two shards: their profiles add up to the whole run's
            c.set_batch(1)
            for fused in (0, 1):
                c.set_option(pocs.OPT_MC_FUSED, fused)
                total, coll = np.zeros(W_SCENE, dtype=np.uint64), 0
                for first, count in ((0, 1000), (1000, 1500)):
                    c.set_shard(first, count)
                    c.set_seed(SEED)
                    coll += c.mc_run_local()
                    total += c.mc_waypoint_counts()
                    xyz, hits = c.particles(count)
                    assert np.array_equal(xyz, want["xyz"][first:first + count]) and np.array_equal(hits, want["hits"][first:first + count])
                c.set_shard()
                assert np.array_equal(total, want["profile"]) and coll == want["collided"], fused


@pytest.mark.gpu
def test_plans_each_on_their_own_clock(pocs, orc, scene):
    N = N_MC
    plans = [prefix(scene["plan"], w) for w in (9, 5, 1)]
    alone = []
    for pl in plans:                                      # the same plan alone on a fresh context under the same schedule
        with context(pocs, scene, N, plan=pl) as c:
            alone.append(run_both(c, pocs, N))
    full = composed_gmm(orc, plans[0], scene["fp"], scene["sched"], SEED, N)
    prof = [composed_mc(orc, pl, scene["fp"], scene["sched"], SEED, N)["profile"] for pl in plans]
    assert is_composed(alone[0]["gmm"], alone[0]["p"], full)
    with context(pocs, scene, N) as c:
        c.set_option(pocs.OPT_PLAN_SEEDS, 1)
        c.set_option(pocs.OPT_MC_WAYPOINT_COUNTS, 1)
        c.set_plans(plans)
        c.set_seed(SEED)
        p0 = c.run_gmm_estimation()
        finals = c.batch_probabilities().copy()
        assert p0 == finals[0]
        for i in range(3):
            c.select_batch_run(i)
            assert finals[i] == alone[i]["p"] and same(gmm_view(c), alone[i]["gmm"]), i
        for fused in (0, 1):
            c.set_option(pocs.OPT_MC_FUSED, fused)
            c.set_seed(SEED)
            c.run_simulation()
            counts = c.mc_batch_counts()
            for i in range(3):
                c.select_batch_run(i)
                a = alone[i]["mc%d" % fused]
                assert counts[i] == int(a["counts"][0]) and np.array_equal(c.mc_waypoint_counts(), a["wp"]), (i, fused)
                assert np.array_equal(c.mc_waypoint_counts(), prof[i]), (i, fused)
                xyz, hits = c.particles(N)
                assert np.array_equal(xyz, a["xyz"]) and np.array_equal(hits, a["hits"]), (i, fused)
        # the GMM risk bound on top: it reads counts, not worlds
        print("composed running probability:", full["running"].tolist())
        assert full["running"][2] < 0.3 <= full["running"][3]
        c.set_plan_risk_bound(0.3)
        c.set_seed(SEED)
        c.run_gmm_estimation()
        E = c.plan_evaluated()
        assert E[0] == 4 and c.batch_probabilities()[0] == full["running"][3]
        c.select_batch_run(0)
        assert np.array_equal(c.waypoint_probabilities(), full["probs"][:4])
        # the MC stop: where the composed counts say, by the rule of pocs.h
        c.set_option(pocs.OPT_MC_RISK_BOUND, 1)
        for fused in (0, 1):                              # (a call that stops takes the per-step form either way)
            c.set_option(pocs.OPT_MC_FUSED, fused)
            c.set_seed(SEED)
            c.run_simulation()
            E, counts = c.plan_evaluated(), c.mc_batch_counts()
            for i in range(3):
                e, coll = mc_stop(prof[i], N, 0.3)
                c.select_batch_run(i)
                assert E[i] == e and counts[i] == coll and np.array_equal(c.mc_waypoint_counts(), prof[i][:e]), (i, fused)
        assert mc_stop(prof[0], N, 0.3)[0] < 9            # (the bound does stop the long plan)


@pytest.mark.gpu
def test_tree_nodes_see_the_world_of_their_depth(pocs, scene):
    N = N_MC
    parent, poses, odoms, leaf = pocs.tree_from_plans([scene["plan"], branch(pocs, scene["plan"], 3, 0.05)])
    T = len(parent)
    assert T == 9 + 5
    with context(pocs, scene, N) as c:
        c.set_option(pocs.OPT_PLAN_SEEDS, 1)
        c.set_plan_tree(parent, poses, odoms)
        c.set_seed(SEED)
        c.run_gmm_estimation()
        probs = c.tree_probabilities().copy()
        views = []
        for n in range(T):
            c.select_tree_node(n)
            views.append(gmm_view(c))
        counts, wps = {}, {}
        for fused in (0, 1):
            c.set_option(pocs.OPT_MC_FUSED, fused)
            c.set_seed(SEED)
            c.run_simulation()
            counts[fused] = c.tree_counts().copy()
            wps[fused] = []
            for n in range(T):
                c.select_tree_node(n)
                wps[fused].append(c.mc_waypoint_counts().copy())
    assert len(set(probs[leaf].tolist())) == 2
    with context(pocs, scene, N) as ref:
        ref.set_option(pocs.OPT_PLAN_SEEDS, 1)
        ref.set_option(pocs.OPT_MC_WAYPOINT_COUNTS, 1)
        for n in range(T):
            ref.set_plans([pocs.tree_path(parent, poses, odoms, n)])
            ref.set_seed(SEED)
            p = ref.run_gmm_estimation()
            assert probs[n] == p and same(views[n], gmm_view(ref)), n
            for fused in (0, 1):
                ref.set_option(pocs.OPT_MC_FUSED, fused)
                ref.set_seed(SEED)
                ref.run_simulation()
                assert counts[fused][n] == ref.mc_batch_counts()[0] and np.array_equal(wps[fused][n], ref.mc_waypoint_counts()), (n, fused)
            ref.clear_plans()


@pytest.mark.gpu
def test_bad_schedules_are_refused_and_change_nothing(pocs, scene):
    N = N_MC
    dp = C.POINTER(C.c_double)
    with context(pocs, scene, N) as c:
        before = run_both(c, pocs, N)
        ok = np.ascontiguousarray(scene["sched"])
        big = np.ones((2, 65, 5))
        nan = ok.copy()
        nan[3, 1, 0] = np.nan
        inf = ok.copy()
        inf[6, 3, 4] = np.inf
        flat = ok.copy()
        flat[2, 0, 2] = 0.0
        long = np.ones((4097, 1, 5))
        for boxes, M, S in ((big.ctypes.data_as(dp), 65, 2), (ok.ctypes.data_as(dp), 4, 0), (long.ctypes.data_as(dp), 1, 4097),
                            (nan.ctypes.data_as(dp), 4, 7), (inf.ctypes.data_as(dp), 4, 7), (flat.ctypes.data_as(dp), 4, 7),
                            (None, 4, 7), (ok.ctypes.data_as(dp), -1, 7), (ok.ctypes.data_as(dp), 4, -1)):
            assert c.lib.pocs_set_obstacle_schedule(c.h, boxes, M, S) == pocs.capi.E_ARG, (M, S)
            assert c.world_steps() == 7
        with pytest.raises(ValueError):
            c.set_obstacle_schedule(np.zeros((7, 4, 4)))
        assert same_runs(run_both(c, pocs, N), before)    # the context still runs the world it had
