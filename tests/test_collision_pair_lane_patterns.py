"""The two-pose footprint test (pocs_pair_loop) on chosen LANE PATTERNS, against the oracle.

pocs_probe_device_collide pairs poses 2 p and 2 p + 1 in thread p of one block, so a test decides which lanes of a wave hold
which pose of their pair in which record's broad-phase box -- what the pair loop's wave-uniform branches see, and what any
form of it that shares work between the two poses has to get right (one narrow pass for both poses where no lane holds both
in a box was built on these cases, gave the oracle's flags on all of them and was measured slower than the two-pose pass:
DESIGN.md section 5; it is not in the tree, the cases stay):

  (a) record A with even lanes' pose 0 and odd lanes' pose 1 in its box: true touches, poses the obstacle's axes separate,
      poses only the footprint's axes separate (a corner grazed): the two masks are disjoint
  (b) the same with one lane holding both poses in the box
  (c) A (disjoint), B' (the same lanes inside with the same pose, others with pose 0 only), then B, which holds the OTHER pose
      of lanes that were inside A, and a record behind B; and the table [A, B'] alone
  (d) (a) with a turned record            (e) (a) with an offset footprint
  (f) every record out of the mixture's reach: the kept list is empty, every flag 0

lane_states() names what a loop that merged the two poses' passes would do per record ("merged" while every lane inside a
box is inside with one and the same pose, "full" from the first record where that fails): the cases are asserted to be the
ones they name by recomputing the broad-phase masks here from the records the device kept.

Each case: flag_full == flag_pair == flag_pair_eager == the oracle's predicate, on every pose.  Not vacuous: (a) - (e) hold at
least 8 pairs with a pose inside a box and at least 2 true touches ((f) has no box left to be inside of: there the kept list
is asserted empty although the table is not).  Then 20 seeds x 512 random poses around the bundled room's walls."""
import ctypes as C
import math

import numpy as np
import pytest

PI = math.pi
FAR = 50.0                                      # a pose out of every box's reach
FP = (0.0, 0.0, 0.3, 0.1)
FP_OFFSET = (0.2, -0.1, 0.3, 0.1)
BOX_A = [0.0, 0.0, 1.0, 0.5, 0.0]
BOX_B1 = [2.2, 0.0, 1.0, 0.5, 0.0]              # B': its broad-phase box overlaps A's for 0.884 <= x <= 1.316
BOX_B = [0.0, 10.0, 1.0, 0.5, 0.0]
BOX_C = [0.0, -10.0, 1.0, 0.5, 0.0]             # a record behind B


def oracle_flags(orc, fp, boxes, poses):
    fp_a = (C.c_double * 4)(*fp)
    b = np.ascontiguousarray(boxes, dtype=np.float64).reshape(-1, 5)
    bp = b.ctypes.data_as(C.POINTER(C.c_double))
    return np.array([bool(orc.lib.orc_collides(C.c_double(x), C.c_double(y), C.c_double(t), fp_a, bp, b.shape[0])) for x, y, t in poses])


def wide_mixture():
    """K = 1, a reach that holds every pose of this file and every heading: the cull keeps every record."""
    p = np.zeros((1, 12))
    p[0, 3:9] = [100.0, 0.0, 100.0, 0.0, 0.0, 1000.0]
    return p


def in_box(kept, fp, poses):
    """pocs_box_hit's broad phase per pose and kept record, as the device evaluates it for a centred footprint (an offset
    footprint: with numpy's sine and cosine, which is as good away from a box's edge): bool[n, nkeep]."""
    c, s = np.cos(poses[:, 2]), np.sin(poses[:, 2])
    px = poses[:, 0] + (c * fp[0] - s * fp[1] if (fp[0] or fp[1]) else 0.0)
    py = poses[:, 1] + (s * fp[0] + c * fp[1] if (fp[0] or fp[1]) else 0.0)
    return ~(np.abs(kept[None, :, 0] - px[:, None]) > kept[None, :, 6]) & ~(np.abs(kept[None, :, 1] - py[:, None]) > kept[None, :, 7])


def margins(fp, box, pose):
    """(largest margin on the obstacle's two axes, on the footprint's two): > 0 = separated there (plain floating point: the
    poses that use it lie 1e-2 from every boundary)."""
    x, y, th = pose
    cx, cy, hx, hy, yaw = box
    px = x + math.cos(th) * fp[0] - math.sin(th) * fp[1]
    py = y + math.sin(th) * fp[0] + math.cos(th) * fp[1]
    dx, dy, rel = cx - px, cy - py, th - yaw
    cr, sr = abs(math.cos(rel)), abs(math.sin(rel))
    e1 = dx * math.cos(yaw) + dy * math.sin(yaw)
    e2 = dy * math.cos(yaw) - dx * math.sin(yaw)
    d1 = dx * math.cos(th) + dy * math.sin(th)
    d2 = dy * math.cos(th) - dx * math.sin(th)
    return (max(abs(e1) - (hx + fp[2] * cr + fp[3] * sr), abs(e2) - (hy + fp[2] * sr + fp[3] * cr)),
            max(abs(d1) - (fp[2] + hx * cr + hy * sr), abs(d2) - (fp[3] + hx * sr + hy * cr)))


def near_a_box(box, kind, j):
    """A pose in the box's own frame moved into the world: 'touch' inside the box, 'obstacle' beside its long face within the
    broad phase's reach but separated by the box's x axis, 'corner' at 45 degrees off a corner where only the footprint's
    own axis separates; j varies the place."""
    cx, cy, hx, hy, yaw = box
    f = 0.01 * (j % 7)
    if kind == "touch":
        u, v, t = (-0.8 + 0.23 * (j % 8)) * hx, (0.9 - 0.3 * (j % 5)) * hy, 0.37 * j
    elif kind == "obstacle":
        u, v, t = (hx + 0.25 + f) * (1 if j % 2 else -1), 0.1 * hy, PI / 2      # the footprint 0.1 wide along the box's x: 0.15 clear
    else:
        a = 0.23 + 0.5 * f                                                        # 0.2121 < a < 0.283
        u, v, t = hx + a, hy + a, PI / 4
    c, s = math.cos(yaw), math.sin(yaw)
    return (cx + c * u - s * v, cy + s * u + c * v, t + yaw)


def far_pose(j):
    return (FAR + 0.5 * j, -FAR - 0.25 * j, 0.1 * j)


def case_a(box=BOX_A, fp=FP, npairs=64):
    """Even lanes: pose 0 in the box, odd lanes: pose 1; the other pose far away."""
    poses = []
    for p in range(npairs):
        near = near_a_box(box, ("touch", "obstacle", "corner")[(p // 2) % 3], p)
        poses += [near, far_pose(p)] if p % 2 == 0 else [far_pose(p), near]
    return np.array(poses)


def case_c(npairs=64):
    """lane % 4 == 0: pose 0 in A      1: pose 1 in A, pose 0 in B (the OTHER pose of a selected lane) for every third such lane
               2: pose 0 in B' only   3: pose 1 in A AND in B' (x in the overlap of their broad-phase boxes)"""
    poses = []
    for p in range(npairs):
        kind = ("touch", "obstacle", "corner")[(p // 4) % 3]
        if p % 4 == 0:
            poses += [near_a_box(BOX_A, kind, p), far_pose(p)]
        elif p % 4 == 1:
            other = near_a_box(BOX_B, kind, p) if (p // 4) % 3 == 0 else far_pose(p)
            poses += [other, near_a_box(BOX_A, kind, p)]
        elif p % 4 == 2:
            poses += [near_a_box(BOX_B1, kind, p), far_pose(p)]
        else:
            poses += [far_pose(p), (1.0 + 0.01 * (p % 20), 0.3 - 0.02 * (p % 9), 0.3 * p)]
    return np.array(poses)


def run_case(ctx, orc, name, fp, boxes, params, poses, min_in_box=8, min_touches=2):
    boxes = np.array(boxes, dtype=np.float64).reshape(-1, 5)
    ctx.set_env(dict(footprint=fp, boxes=boxes))
    full, pair, eager, kept = ctx.probe_device_collide(params, poses)
    want = oracle_flags(orc, fp, boxes, poses)
    for what, got in (("full", full), ("pair", pair), ("pair, eager", eager)):
        bad = np.flatnonzero(got != want.astype(np.int32))
        assert bad.size == 0, (name, what, len(bad), [(int(i), tuple(poses[i]), int(got[i]), bool(want[i])) for i in bad[:5]])
    inb = in_box(kept, fp, poses) if len(kept) else np.zeros((len(poses), 0), dtype=bool)
    pairs_in = int((inb[0::2].any(axis=1) | inb[1::2].any(axis=1)).sum())
    assert pairs_in >= min_in_box and int(want.sum()) >= min_touches, (name, pairs_in, int(want.sum()))
    return kept, inb, want


def lane_states(inb):
    """Per wave of 64 pairs and kept record, from the broad-phase masks: 'none' (no lane inside a box so far), 'merged' (every lane
    inside a box so far was inside with one and the same pose), 'full' (some lane has had both poses inside)."""
    out = []
    for w0 in range(0, inb.shape[0] // 2, 64):
        pm0, pm1 = inb[0::2][w0:w0 + 64], inb[1::2][w0:w0 + 64]
        state, sel, trail = "none", None, []
        for m in range(inb.shape[1]):
            a, b = pm0[:, m], pm1[:, m]
            if (a | b).any() and state != "full":
                if state == "none":
                    state, sel = ("merged", b.copy()) if not (a & b).any() else ("full", None)
                elif (b & ~sel).any() or (a & sel).any():
                    state = "full"
            trail.append(state)
        out.append(trail)
    return out


@pytest.mark.gpu
def test_pair_lane_pattern_cases_equal_the_oracle(pocs, orc):
    wide = wide_mixture()
    with pocs.Context(0) as ctx:
        # (a) one wave, and all eight
        for npairs in (64, 512):
            poses = case_a(npairs=npairs)
            kept, inb, want = run_case(ctx, orc, "(a) %d pairs" % npairs, FP, [BOX_A], wide, poses)
            assert len(kept) == 1 and not (inb[0::2, 0] & inb[1::2, 0]).any()
            assert inb[0::4, 0].all() and inb[3::4, 0].all() and not inb[1::4, 0].any() and not inb[2::4, 0].any()
            assert lane_states(inb) == [["merged"]] * (npairs // 64)
            kinds = {"touch": 0, "obstacle": 0, "corner": 0}
            for i in np.flatnonzero(inb[:, 0]):
                mo, mf = margins(FP, BOX_A, poses[i])
                k = "obstacle" if mo > 1e-2 else "corner" if mo < -1e-2 and mf > 1e-2 else "touch" if mo < -1e-2 and mf < -1e-2 else "?"
                assert (k == "touch") == bool(want[i]), (i, poses[i], mo, mf)
                kinds[k] += 1
            assert min(kinds.values()) >= 8 and set(kinds) == {"touch", "obstacle", "corner"}, kinds
        # (b) lane 5 holds both poses in the box
        poses = case_a()
        poses[10] = near_a_box(BOX_A, "touch", 3)
        poses[11] = near_a_box(BOX_A, "corner", 4)
        kept, inb, _ = run_case(ctx, orc, "(b)", FP, [BOX_A], wide, poses)
        assert int((inb[0::2, 0] & inb[1::2, 0]).sum()) == 1 and lane_states(inb) == [["full"]]
        # (c) the state changes at B, behind a B' that left it merged; and [A, B'] alone
        poses = case_c()
        kept, inb, _ = run_case(ctx, orc, "(c) A B' B C", FP, [BOX_A, BOX_B1, BOX_B, BOX_C], wide, np.vstack([poses, case_a(BOX_C, npairs=8)]))
        assert len(kept) == 4 and lane_states(inb[:128]) == [["merged", "merged", "full", "full"]]
        assert inb[:128, 1].sum() >= 16 and inb[:128, 2].sum() >= 4 and inb[128:, 3].sum() >= 8
        assert (inb[1:128:2, 0] & inb[1:128:2, 1]).sum() >= 8          # lanes whose selected pose is in A's box and in B''s
        kept, inb, _ = run_case(ctx, orc, "(c) A B'", FP, [BOX_A, BOX_B1], wide, poses)
        assert len(kept) == 2 and lane_states(inb) == [["merged", "merged"]]
        # (d) a turned record
        turned = [0.3, -0.2, 1.0, 0.5, 0.4]
        poses = case_a(turned)
        kept, inb, want = run_case(ctx, orc, "(d)", FP, [turned], wide, poses)
        assert kept[0, 2] != 1.0 and kept[0, 3] != 0.0 and lane_states(inb) == [["merged"]]
        seen = set()
        for i in np.flatnonzero(inb[:, 0]):
            mo, mf = margins(FP, turned, poses[i])
            seen.add("obstacle" if mo > 1e-2 else "corner" if mf > 1e-2 else "touch")
        assert seen == {"touch", "obstacle", "corner"}
        # (e) an offset footprint: the poses of (a) moved so that the footprint's centre is where it was
        poses = case_a(fp=FP_OFFSET)
        c, s = np.cos(poses[:, 2]), np.sin(poses[:, 2])
        poses[:, 0] -= c * FP_OFFSET[0] - s * FP_OFFSET[1]
        poses[:, 1] -= s * FP_OFFSET[0] + c * FP_OFFSET[1]
        kept, inb, _ = run_case(ctx, orc, "(e)", FP_OFFSET, [BOX_A], wide, poses)
        assert len(kept) == 1 and not (inb[0::2, 0] & inb[1::2, 0]).any()
        # (f) a mixture that reaches no record: nothing kept, no flag set
        narrow = np.zeros((1, 12))
        narrow[0, :3] = [20.0, 20.0, 0.3]
        narrow[0, 3:9] = [0.01, 0.0, 0.01, 0.0, 0.0, 0.01]
        rng = np.random.default_rng(7)
        poses = narrow[0, :3] + rng.uniform(-0.05, 0.05, (128, 3))
        kept, _, want = run_case(ctx, orc, "(f)", FP, [BOX_A, BOX_B1, BOX_B, [0.3, -0.2, 1.0, 0.5, 0.4]], narrow, poses, 0, 0)
        assert len(kept) == 0 and not want.any()


def room_poses(env, hh, seed, spread):
    """512 poses, each around a wall picked at random: uniform in the wall's broad-phase box scaled by `spread`."""
    rng = np.random.default_rng(seed)
    boxes, fp = env["boxes"], env["footprint"]
    fp_a = (C.c_double * 4)(*fp)
    rec = np.zeros((len(boxes), 8))
    for m, b in enumerate(np.ascontiguousarray(boxes, dtype=np.float64)):
        hh.hh_prepare_obstacle(b.ctypes.data_as(C.POINTER(C.c_double)), fp_a, rec[m].ctypes.data_as(C.POINTER(C.c_double)))
    m = rng.integers(0, len(boxes), 512)
    poses = np.stack([rec[m, 0] + spread * rec[m, 6] * rng.uniform(-1, 1, 512), rec[m, 1] + spread * rec[m, 7] * rng.uniform(-1, 1, 512),
                      rng.uniform(-7, 7, 512)], axis=1)
    return poses, rec


@pytest.fixture(scope="module")
def room_sweep(env, hh):
    """The sweep's poses, built once on the CPU: the spread is the first of a fixed list at which 5 - 20 % of every seed's poses
    lie in some record's broad-phase box (the table's, for a centred footprint: the cull of a wide mixture keeps it)."""
    assert env["footprint"][0] == 0.0 and env["footprint"][1] == 0.0
    for spread in (2.0, 2.5, 3.0, 3.5, 4.0, 5.0, 6.0):
        sets, ok = [], True
        for seed in range(20):
            poses, rec = room_poses(env, hh, 9100 + seed, spread)
            frac = in_box(rec, env["footprint"], poses).any(axis=1).mean()
            ok = ok and 0.05 <= frac <= 0.20
            sets.append(poses)
        if ok:
            return spread, sets
    raise AssertionError("no spread of the list puts 5 - 20 % of every seed's poses in a box")


def test_room_sweep_poses_are_in_a_box_often_enough(room_sweep, env, hh, orc):
    spread, sets = room_sweep
    assert len(sets) == 20 and all(s.shape == (512, 3) for s in sets)
    hits = sum(int(oracle_flags(orc, env["footprint"], env["boxes"], s).sum()) for s in sets[:3])
    assert 0 < hits < 3 * 512, (spread, hits)


@pytest.mark.gpu
def test_pair_random_poses_around_the_room_walls(pocs, orc, env, room_sweep):
    _, sets = room_sweep
    wide = wide_mixture()
    compared = merged = 0
    with pocs.Context(0) as ctx:
        ctx.set_env(env)
        for poses in sets:
            full, pair, eager, kept = ctx.probe_device_collide(wide, poses)
            want = oracle_flags(orc, env["footprint"], env["boxes"], poses).astype(np.int32)
            assert len(kept) == len(env["boxes"])
            for what, got in (("full", full), ("pair", pair), ("pair, eager", eager)):
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, (what, len(bad), [(int(i), tuple(poses[i])) for i in bad[:5]])
            compared += len(want)
            merged += sum("merged" in t for t in lane_states(in_box(kept, env["footprint"], poses)))
    assert compared == 20 * 512                      # no pose left out
    assert merged >= 20                              # of the 80 waves, those with disjoint masks at their first record inside a box
