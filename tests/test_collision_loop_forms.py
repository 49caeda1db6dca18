"""The sampling loop's footprint test in each of its forms, bit for bit against the CPU oracle (`==`, as test_gpu_parity.py).

k_gmm_step hands the two poses of a thread's pair to one pass over the culled obstacle table that fetches a record once
for both poses, keeps the collision flags as lane masks in scalar registers, computes the headings' sines and cosines only
once some lane is inside a record's broad-phase box (a centred footprint) or in front of the loop (an offset one), and has
a counting form (per-box counts) and heads that commit a large world's records.  The shapes are the smallest at which these
paths can go wrong: K = 3, W = 3, N = 2 * 1024 + 130 -- the last chunk partial, component boundaries inside a wave (so the
general form of the iteration runs next to the whole-wave form), and with an odd shard the pair's unused twin.

Every case compares samples, flags, moments and per-waypoint probabilities; a case whose call holds no collided sample, or no
collision-free one, at any waypoint fails (the oracle alone satisfies that for cases 2-6: checked without a GPU below)."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

gpu = pytest.mark.gpu
SEED = 0x5EED0001
WEYL = 0x9E3779B97F4A7C15
K, W, N = 3, 3, 2 * 1024 + 130
SHARD = (2 * 37, N - 2 * 37 - 1)                     # an even start, an ODD count: the last pair's second slot is unused
START_WALLS = 25                                     # waypoints 25 .. 27 of the bundled plan: the turn next to the inner wall
START_TURNED = 0                                     # waypoints 0 .. 2: the room's corner, between a wall and the first slat
GOLDEN = Path(__file__).with_name("golden")
_dp = C.POINTER(C.c_double)
_cache = {}


def sub_plan(plan, start):
    return dict(traj=plan["traj"][start:start + W], odom=plan["odom"][start:start + W - 1])


def scene(pocs, plan, env, case):
    """(plan, env) of a case: the oracle's world; `world` (case 6) is what the GPU gets through set_world instead."""
    room = np.asarray(env["boxes"], np.float64).reshape(-1, 5)
    if case == "nothing":
        return sub_plan(plan, START_WALLS), dict(footprint=env["footprint"], boxes=np.array([[50.0, 50.0, 0.1, 0.1, 0.3]]))
    if case == "walls":
        return sub_plan(plan, START_WALLS), dict(footprint=env["footprint"], boxes=room)
    if case == "turned":
        e = pocs.load_env(str(GOLDEN / "pr2custom_env.txt"))
        return sub_plan(plan, START_TURNED), dict(footprint=e["footprint"], boxes=np.asarray(e["boxes"], np.float64).reshape(-1, 5))
    if case == "offset":
        fp = list(env["footprint"])
        fp[0], fp[1] = 0.05, -0.02
        return sub_plan(plan, START_WALLS), dict(footprint=fp, boxes=room)
    if case == "large":
        rng = np.random.default_rng(11)
        n = 65 - len(room)
        far = np.column_stack([rng.uniform(20.0, 60.0, n), rng.uniform(-2.0, 2.0, n), rng.uniform(0.05, 0.4, n), rng.uniform(0.05, 0.4, n),
                               np.where(rng.random(n) < 0.3, 0.0, rng.uniform(-3.2, 3.2, n))])
        return sub_plan(plan, START_WALLS), dict(footprint=env["footprint"], boxes=rng.permutation(np.vstack([room, far]), axis=0))
    raise KeyError(case)


def reference(pocs, orc, plan, env, case, seed=SEED):
    """The oracle's answers for a case, computed once and left unchanged: the free-running call (moments, probabilities, mixtures,
    the last waypoint's samples and flags), every waypoint's samples and flags, and waypoint 0 of the odd shard."""
    key = (case, seed)
    if key not in _cache:
        pl, e = scene(pocs, plan, env, case)
        cfg = orc.config(pl, e, K=K)
        want = orc.run_gmm(cfg, seed, N, want_samples=True)
        per_w = [orc.gmm_waypoint(cfg, seed, w, want["states"][w], 0, N, want_samples=True) for w in range(W)]
        for w in range(W):
            assert np.array_equal(per_w[w][0], want["moments"][w])
        assert np.array_equal(per_w[W - 1][1], want["samples"]) and np.array_equal(per_w[W - 1][2], want["flags"])
        shard = orc.gmm_waypoint(cfg, seed, 0, want["states"][0], SHARD[0], SHARD[1], want_samples=True, n_total=N)
        _cache[key] = dict(plan=pl, env=e, cfg=cfg, want=want, per_w=per_w, shard=shard)
    return _cache[key]


def not_vacuous(ref):
    """Some waypoint of the call has a collided sample and some waypoint a collision-free one -- and so has the shard's waypoint 0."""
    coll = ref["want"]["moments"][:, :, 1].sum(axis=1)
    free = ref["want"]["moments"][:, :, 0].sum(axis=1)
    sf = ref["shard"][2]
    return bool(coll.max() > 0 and free.max() > 0 and 0 < int(sf.astype(bool).sum()) < len(sf))


def touched(orc, xyz, fp, boxes):
    """(n, M) bool: the oracle's predicate for every pose against every single box."""
    fpa = np.ascontiguousarray(fp, np.float64)
    b = np.ascontiguousarray(boxes, np.float64).reshape(-1, 5)
    recs = [C.cast(b.ctypes.data + 5 * 8 * m, _dp) for m in range(len(b))]
    f, one, cd, pf = orc.lib.orc_collides, C.c_int(1), C.c_double, fpa.ctypes.data_as(_dp)
    out = np.zeros((len(xyz), len(b)), dtype=bool)
    for i, (x, y, t) in enumerate(np.asarray(xyz, np.float64).tolist()):
        for m, r in enumerate(recs):
            if f(cd(x), cd(y), cd(t), pf, r, one):
                out[i, m] = True
    return out


def inside_tight_box(xyz, fp, boxes):
    """(n, M) bool: the pose's base point inside the box's own world AABB grown by the footprint's SMALLEST half extent -- inside
    every broad-phase box the kernel can give the record (the culled table's is the AABB grown by the footprint's extent over the
    run's headings, never less than that), and a record with such a sample is kept by the cull: the narrow phase runs for it.
    (A centred footprint.)"""
    b = np.asarray(boxes, np.float64).reshape(-1, 5)
    r = min(fp[2], fp[3])
    ax = b[:, 2] * np.abs(np.cos(b[:, 4])) + b[:, 3] * np.abs(np.sin(b[:, 4]))
    ay = b[:, 2] * np.abs(np.sin(b[:, 4])) + b[:, 3] * np.abs(np.cos(b[:, 4]))
    return (np.abs(xyz[:, None, 0] - b[None, :, 0]) <= ax + r) & (np.abs(xyz[:, None, 1] - b[None, :, 1]) <= ay + r)


def both_narrow_branches(ref):
    """Within the call, some pose reaches the narrow phase of an axis-aligned record and some pose that of a turned one."""
    b = ref["env"]["boxes"]
    aligned = (np.cos(b[:, 4]) == 1.0) & (np.sin(b[:, 4]) == 0.0)
    hit = np.zeros(len(b), bool)
    for _, xyz, _, _ in ref["per_w"]:
        hit |= inside_tight_box(xyz, ref["env"]["footprint"], b).any(axis=0)
    return bool(hit[aligned].any() and hit[~aligned].any())


# ---- without a GPU: the inputs are what the cases need, by the oracle alone ---------------------------------------------------

def test_the_oracle_alone_satisfies_the_cap(pocs, orc, plan, env):
    for case in ("walls", "turned", "offset", "large"):
        assert not_vacuous(reference(pocs, orc, plan, env, case)), case
    nothing = reference(pocs, orc, plan, env, "nothing")
    assert nothing["want"]["moments"][:, :, 1].sum() == 0 and not nothing["want"]["flags"].any()
    assert both_narrow_branches(reference(pocs, orc, plan, env, "turned"))
    off = reference(pocs, orc, plan, env, "offset")
    assert off["env"]["footprint"][0] != 0.0 and off["env"]["footprint"][1] != 0.0
    # the large world is the walls' world plus boxes out of every pose's reach: the same answers
    large, walls = reference(pocs, orc, plan, env, "large"), reference(pocs, orc, plan, env, "walls")
    assert len(large["env"]["boxes"]) == 65
    assert np.array_equal(large["want"]["moments"], walls["want"]["moments"]) and np.array_equal(large["want"]["flags"], walls["want"]["flags"])
    # component boundaries inside a wave: no component's block of samples starts or ends on a multiple of 128
    comp = walls["per_w"][0][3]
    edges = np.flatnonzero(np.diff(comp.astype(int))) + 1
    assert len(edges) == K - 1 and all(e % 128 for e in edges) and N % 1024 != 0


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------

def call_outputs(c):
    xyz, flags = c.gmm_samples(N)
    return dict(probs=c.waypoint_probabilities().copy(), moments=np.array([c.moments(w, K) for w in range(W)]),
                states=np.array([c.gmm_state_raw(w, K) for w in range(W)]), xyz=xyz.copy(), flags=flags.copy())


def check_call(got, p, want):
    assert np.array_equal(got["flags"], want["flags"]), "flags"
    assert np.array_equal(got["xyz"], want["samples"]), "samples"
    assert np.array_equal(got["moments"], want["moments"]), "moments"
    assert np.array_equal(got["probs"], want["probs"]) and p == want["prob"], "probabilities"
    assert np.array_equal(got["states"], want["states"]), "mixtures"


def check_odd_shard(c, ref, seed=SEED):
    """Waypoint 0 of the odd shard through the step API: its samples, flags and moments are the oracle's for that index range."""
    c.set_seed(seed)
    c.set_shard(*SHARD)
    try:
        c.gmm_begin()
        c.gmm_step_local(0)
        xyz, flags = c.gmm_samples(SHARD[1])
        for w in range(1, W):
            c.gmm_step_local(w)
        c.gmm_end()
        got = c.moments(0, K)
    finally:
        c.set_shard()
    mom, samples, oflags, _ = ref["shard"]
    assert np.array_equal(flags, oflags) and np.array_equal(xyz, samples) and np.array_equal(got, mom)


def run_case(pocs, ref):
    with pocs.Context(0) as c:
        c.configure(ref["plan"], ref["env"], K=K, N=N, seed=SEED)
        p = c.run_gmm_estimation()
        got = call_outputs(c)
        check_call(got, p, ref["want"])
        check_odd_shard(c, ref)
    return got


@gpu
def test_a_world_with_nothing_in_reach(pocs, orc, plan, env):
    ref = reference(pocs, orc, plan, env, "nothing")
    got = run_case(pocs, ref)
    assert not got["flags"].any() and np.all(got["moments"][:, :, 1] == 0) and np.all(got["moments"][:, :, 0].sum(axis=1) == N)


@gpu
def test_the_bundled_walls_lone_form_and_run_0_of_a_batch(pocs, orc, plan, env):
    ref = reference(pocs, orc, plan, env, "walls")
    assert not_vacuous(ref)
    lone = run_case(pocs, ref)                                          # one run per call: the lone form
    with pocs.Context(0) as c:
        c.configure(ref["plan"], ref["env"], K=K, N=N, seed=SEED)
        c.set_batch(3)
        p0 = c.run_gmm_estimation()
        finals = list(c.batch_probabilities())
        c.select_batch_run(0)
        batch = call_outputs(c)
        check_call(batch, p0, ref["want"])
        assert all(np.array_equal(batch[k], lone[k]) for k in lone)
        c.select_batch_run(2)                                           # and the batch's last run on its own effective seed
        r2 = reference(pocs, orc, plan, env, "walls", (SEED + 2 * WEYL) % 2 ** 64)
        check_call(call_outputs(c), finals[2], r2["want"])


@gpu
def test_a_world_of_turned_boxes(pocs, orc, plan, env):
    ref = reference(pocs, orc, plan, env, "turned")
    assert not_vacuous(ref) and both_narrow_branches(ref)
    run_case(pocs, ref)


@gpu
def test_an_offset_footprint(pocs, orc, plan, env):
    ref = reference(pocs, orc, plan, env, "offset")
    assert not_vacuous(ref)
    run_case(pocs, ref)


@gpu
def test_the_counting_form(pocs, orc, plan, env):
    ref = reference(pocs, orc, plan, env, "walls")
    assert not_vacuous(ref)
    boxes, fp = ref["env"]["boxes"], ref["env"]["footprint"]
    want_counts = np.array([touched(orc, xyz, fp, boxes).sum(axis=0) for _, xyz, _, _ in ref["per_w"]], dtype=np.uint64)
    for w in range(W):                                                  # what the oracle's flags imply: a flag is set iff some box is touched
        assert np.array_equal(touched(orc, ref["per_w"][w][1], fp, boxes).any(axis=1), ref["per_w"][w][2].astype(bool))
    assert want_counts.sum() > 0
    for batch in (1, 3):                                                # the lone counting form, and the ticket one
        with pocs.Context(0) as c:
            c.configure(ref["plan"], ref["env"], K=K, N=N, seed=SEED)
            c.set_option(pocs.OPT_OBSTACLE_COUNTS, 1)
            c.set_batch(batch)
            p = c.run_gmm_estimation()
            c.select_batch_run(0)
            check_call(call_outputs(c), p, ref["want"])                 # the default form's outputs, unchanged by the option
            got = c.obstacle_counts()
            assert got.shape == (W, len(boxes)) and np.array_equal(got, want_counts), batch


@gpu
def test_a_large_world(pocs, orc, plan, env):
    ref = reference(pocs, orc, plan, env, "large")
    walls = reference(pocs, orc, plan, env, "walls")
    assert not_vacuous(ref)
    with pocs.Context(0) as c:
        c.configure(ref["plan"], walls["env"], K=K, N=N, seed=SEED)
        c.set_world(ref["env"]["boxes"])
        assert c.world_boxes() == 65
        c.set_batch(3)                                                  # (a large world takes the ticket form)
        p = c.run_gmm_estimation()
        c.select_batch_run(0)
        got = call_outputs(c)
        check_call(got, p, ref["want"])
        assert 0 < c.world_reach().max() <= 64
        check_call(got, p, walls["want"])                               # 64 or fewer in reach: the small world's answer
