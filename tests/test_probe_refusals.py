"""The device probes' argument checks and pair walks, pinned probe by probe.

Every probe that takes poses or cases (all but the two sampler-math probes) refuses a literal table of bad inputs with code -1 before
anything reaches the device, and the same context then answers a small valid probe exactly as it did before the refusal.  The valid
probe has three poses -- an odd count, so the last pose is paired with itself -- of which the first touches the one box or disc and the
second does not (pocs_probe_device_disc_noise takes even counts only: four poses there).

A second test per probe gives 130 poses in one call -- more than one wave of pairs, with a last wave of which one lane is live -- and
checks the answer against the probe's own answers for the same poses given one at a time (two at a time, under their own even index,
where the pose index picks the disc noise).  A pair walk with a wrong tail or a wrong lane map shows there and not at three poses.
"""
import numpy as np
import pytest

NAN, INF = float("nan"), float("inf")
FP = [0.1, 0.0, 0.5, 0.25]
BOX = [[2.0, 0.0, 0.5, 0.5, 0.3]]
DISC = [[2.0, 0.0, 0.5]]
COV = [[1e-4, 2e-5, 1e-4]]
POSES = [[1.2, 0.0, 0.0], [-3.0, 1.0, 0.7], [2.0, 0.2, 2.0]]                      # touches, does not, touches
WIDE = [[0.0, 0.0, 0.0, 100.0, 0.0, 100.0, 0.0, 0.0, 1e3, 0.0, 0.0, 0.0]]           # a mixture whose reach holds every pose
VALID = dict(fp=FP, boxes=BOX, discs=DISC, cov=COV, poses=POSES, first=0, kinds=[0], parts=[FP, [-0.6, 0.0, 0.1, 0.1]], params=WIDE,
             K=[2, 1, 3], weights=[[0.25, 0.75] + [0.0] * 6, [1.0] + [0.0] * 7, [0.5, 0.0, 0.5] + [0.0] * 5], n_total=[1000, 7, 4096])


def many(rec, n):
    return [list(rec[0]) for _ in range(n)]


def bad_pose(poses=POSES):
    p = [list(q) for q in poses]
    p[1][1] = NAN
    return p


ZERO_POSES = ("zero poses", dict(poses=np.zeros((0, 3))))
NAN_POSE = ("a NaN pose coordinate", dict(poses=bad_pose()))
INF_FP = ("an infinite footprint value", dict(fp=[0.1, 0.0, INF, 0.25]))
FLAT_BOX = ("a box with a zero half extent", dict(boxes=[[2.0, 0.0, 0.5, 0.0, 0.3]]))
POINT_DISC = ("a disc with radius 0", dict(discs=[[2.0, 0.0, 0.0]]))
BOXES_65 = ("65 boxes", dict(boxes=many(BOX, 65)))
ODD_FIRST = ("an odd first", dict(first=7))
POSES4 = POSES + [[5.0, 5.0, 1.0]]

# name -> (the call, what only this probe's valid call needs, its bad inputs)
PROBES = {
    "collide": (lambda c, a: c.probe_device_collide(a["params"], a["poses"]), {},
                [ZERO_POSES, NAN_POSE, ("9 components", dict(params=many(WIDE, 9)))]),
    "clearance": (lambda c, a: c.probe_device_clearance(a["fp"], [0.1, 0.3], a["boxes"], a["poses"]), {},
                  [ZERO_POSES, NAN_POSE, INF_FP, FLAT_BOX, BOXES_65]),
    "parts": (lambda c, a: c.probe_footprint_parts(a["parts"], a["boxes"], a["poses"]), {},
              [ZERO_POSES, NAN_POSE, ("an infinite part value", dict(parts=[FP, [-0.6, INF, 0.1, 0.1]])), FLAT_BOX, BOXES_65,
               ("5 parts", dict(parts=many([FP], 5)))]),
    "regions": (lambda c, a: c.probe_device_regions(a["fp"], a["boxes"], a["kinds"], a["poses"]), {},
                [ZERO_POSES, NAN_POSE, INF_FP, FLAT_BOX, ("5 regions", dict(boxes=many(BOX, 5), kinds=[0] * 5))]),
    "segment": (lambda c, a: c.probe_segment(a["fp"], a["boxes"], [0.1, 0.5, -0.1], 4, 0, a["poses"]), {},
                [ZERO_POSES, NAN_POSE, INF_FP, FLAT_BOX, BOXES_65]),
    "discs": (lambda c, a: c.probe_device_discs(a["fp"], a["boxes"], a["discs"], a["poses"]), dict(boxes=[[-2.0, 3.0, 0.5, 0.5, 0.0]]),
              [ZERO_POSES, NAN_POSE, INF_FP, FLAT_BOX, POINT_DISC, ("64 boxes and a disc", dict(boxes=many(BOX, 64)))]),
    "disc_noise": (lambda c, a: c.probe_device_disc_noise(a["fp"], a["discs"], a["cov"], 0x5EED, 3, a["first"], a["poses"]), dict(poses=POSES4),
                   [ZERO_POSES, ("a NaN pose coordinate", dict(poses=bad_pose(POSES4))), INF_FP, POINT_DISC,
                    ("17 discs", dict(discs=many(DISC, 17), cov=many(COV, 17))), ODD_FIRST]),
    "footprint_disc": (lambda c, a: c.probe_device_footprint_disc(a["fp"][2], a["boxes"], a["discs"], a["poses"], a["cov"], 0x5EED, 3, a["first"]),
                       dict(boxes=[[-2.0, 3.0, 0.5, 0.5, 0.0]]),
                       [ZERO_POSES, NAN_POSE, INF_FP, FLAT_BOX, POINT_DISC, ("64 boxes and a disc", dict(boxes=many(BOX, 64))), ODD_FIRST]),
    "counts": (lambda c, a: c.probe_device_counts(a["K"], a["weights"], np.ones((len(a["K"]), 8)), [11, 12, 13][:len(a["K"])],
                                                  [0, 1, 2][:len(a["K"])], a["n_total"]), {},
               [("zero cases", dict(K=[], weights=np.zeros((0, 8)), n_total=[])),
                ("a NaN weight", dict(weights=[[0.25, NAN] + [0.0] * 6, [1.0] + [0.0] * 7, [0.5, 0.0, 0.5] + [0.0] * 5])),
                ("9 components", dict(K=[2, 9, 3]))]),
}


def context(pocs, name):
    c = pocs.Context(0)
    if name == "collide":                                # the one probe that reads the context's world
        c.set_env(dict(footprint=FP, boxes=BOX))
    return c


def parts_of(answer):
    return [np.asarray(p) for p in (answer if isinstance(answer, tuple) else (answer,))]


def same(a, b):
    a, b = parts_of(a), parts_of(b)
    return len(a) == len(b) and all(p.shape == q.shape and np.array_equal(p, q) for p, q in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PROBES))
def test_bad_inputs_are_refused_and_the_context_still_answers(pocs, name):
    call, own, bad = PROBES[name]
    valid = dict(VALID, **own)
    with context(pocs, name) as c:
        first = call(c, valid)
        if name != "counts":                             # pose 0 touches, pose 1 does not: the flags of the probe's main output
            flags = parts_of(first)[1 if name == "disc_noise" else 0]
            free = 2 if name == "clearance" else 0      # (a clearance level: -1 touches, the number of distances for nothing near)
            assert flags[0] != free and flags[1] == free, (name, flags)
        else:                                            # cumulative counts: a case's last component holds its total, zeros behind its K
            assert first.shape == (3, 8) and first[0, 1] == 1000.0 and first[1, 0] == 7.0 and first[2, 2] == 4096.0, first
            assert not first[0, 2:].any() and not first[1, 1:].any() and not first[2, 3:].any(), first
        for label, change in bad:
            with pytest.raises(pocs.PocsError) as e:
                call(c, dict(valid, **change))
            assert e.value.code == -1, (name, label, e.value)
            assert same(call(c, valid), first), (name, label)


def walk_poses(n=130):
    i = np.arange(n, dtype=np.float64)
    return np.stack([0.04 * i - 1.0, 0.3 * np.sin(i), 0.37 * i], axis=1)           # past the box and the disc at x = 2, every heading


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in PROBES if n != "counts"])
def test_130_poses_answer_as_the_same_poses_one_call_each(pocs, name):
    call, own, _ = PROBES[name]
    poses = walk_poses()
    indexed = name in ("disc_noise", "footprint_disc")   # the pose index picks the noise: two poses a call, under their own even index
    step, base = (2, 1 << 20) if indexed else (1, 0)
    valid = dict(VALID, **own)
    with context(pocs, name) as c:
        whole = parts_of(call(c, dict(valid, poses=poses, first=base)))
        if name == "collide":
            whole = whole[:3]                            # (the kept records depend on the mixture alone)
        pieces = [parts_of(call(c, dict(valid, poses=poses[i:i + step], first=base + i)))[:len(whole)] for i in range(0, len(poses), step)]
    main = whole[1 if name == "disc_noise" else 0]
    assert len(np.unique(main)) > 1, (name, "the poses do not tell touching from free", main)
    for j, w in enumerate(whole):
        assert len(w) == len(poses)
        got = np.concatenate([p[j] for p in pieces])
        bad = np.flatnonzero([not np.array_equal(a, b) for a, b in zip(w, got)])
        assert bad.size == 0, (name, j, [(int(i), w[i], got[i]) for i in bad[:5]])
