"""The collision predicate and the obstacle cull of the GMM sampling kernel on the poses where they can go wrong.

Every seeded test compares collision flags of random samples with the oracle: a random pose is never within a few ulps
of touching, and never at the edge of what its mixture can draw.  Here the inputs are picked:

  (a) grazing poses   the flip of the oracle's flag along a ray, located by bisection to adjacent doubles, and the poses
                      at +-1 .. +-6 ulps of the ray parameter around it -- face normals, corner directions, random rays;
                      headings on the quarter turns and the sector ties; box yaws 0, -0, +-pi/2, pi, 2 pi (cos = 1,
                      sin != 0: NOT the axis-aligned shortcut), 1e-17, 2^-30; half extents from 5e-324 to 1.5
  (b) exact touches   dyadic numbers, a margin of exactly 0: must hit, and one ulp further out must miss -- written
                      down by hand, "touching counts as collision" without leaning on the oracle
  (c) reach edge      poses mean_k + L_k z built with the oracle's own chain from the extreme Box-Muller words (radius
                      words 1, 2, 3, 0; the radius on one normal, either sign, and on the diagonal; every sign combination
                      of the three normals), and obstacles bisected against them: an obstacle that touches, or just
                      misses, the footprint at the very edge of what the run can draw, where an error of the cull's
                      bound, bounding box, pad, end values or radius decisions would show
  (d) far obstacles   worlds of 64, 1 and 0 boxes: what lies out of reach is dropped, the rest kept in table order

CPU leg: the host build of pocs_pose_collides (hh_collides) == the oracle on every pose, and the inputs are not vacuous.
GPU leg (pocs_probe_device_collide): the device's three forms of the predicate == the oracle, bit for bit, nothing skipped,
and the kept records are what the cull's comment claims."""
import ctypes as C
import math

import numpy as np
import pytest

PI = math.pi
ULPS = (-6, -5, -4, -3, -2, -1, 0, 1, 2, 3, 4, 5, 6, 7)       # of the ray parameter, from the last hit: 0 hits, 1 misses
C_OFFSETS = (-6, 0, 1, 6)                                      # (c): one world per offset of every obstacle from its last hit
T_FAR = 3.0                                                    # beyond every footprint radius + box radius used here


def collider(fn, fp, boxes):
    """f(x, y, th) -> bool through orc_collides / hh_collides, the world converted once."""
    fp_a = (C.c_double * 4)(*fp)
    b = np.ascontiguousarray(boxes, dtype=np.float64).reshape(-1, 5)
    bp, M = b.ctypes.data_as(C.POINTER(C.c_double)), b.shape[0]

    def f(x, y, th, _keep=b):
        return bool(fn(C.c_double(x), C.c_double(y), C.c_double(th), fp_a, bp, M))
    return f


def step(t, k):
    """t moved by k ulps."""
    for _ in range(abs(k)):
        t = math.nextafter(t, math.inf if k > 0 else -math.inf)
    return t


def bisect_flip(hit_at):
    """hit_at(0) is True, hit_at(T_FAR) False -> the last t that hits, its successor misses."""
    lo, hi = 0.0, T_FAR
    assert hit_at(lo) and not hit_at(hi)
    while math.nextafter(lo, hi) != hi:
        mid = lo + 0.5 * (hi - lo)
        if hit_at(mid):
            lo = mid
        else:
            hi = mid
    return lo


# ---------------------------------------------------------------------------------------------------------------
# (a) grazing poses
# ---------------------------------------------------------------------------------------------------------------
FOOTPRINTS = [("centred square", (0.0, 0.0, 0.25, 0.25)), ("offset square", (0.3, -0.2, 0.25, 0.25)),
              ("centred 10:1", (0.0, 0.0, 0.5, 0.05)), ("offset 10:1", (-0.25, 0.3, 0.05, 0.5)),
              ("tiny", (0.0, 0.0, 1e-150, 3e-151))]      # (the squares in its bounding radius still above the underflow)
HEADINGS = ([0.0, PI / 2, -PI / 2, PI, PI / 4] + [k * PI / 2 for k in range(-8, 9)] +
            [(j + 0.5) * PI / 128 for j in (-200, -129, -65, -1, 0, 31, 63, 64, 127, 199)] + [123456.789, -99999.5])
YAWS = [0.0, -0.0, PI / 2, -PI / 2, PI, 2 * PI, 1e-17, 2.0 ** -30]
EXTENTS = [5e-324, 1e-300, 1e-9, 0.02, 0.25, 1.0, 1.5]
GRID = [(8.0 * i, 8.0 * j) for j in (-1, 0, 1) for i in (-1.5, -0.5, 0.5, 1.5)]      # box centres, out of each other's reach


def grazing_cases(orc):
    rng = np.random.default_rng(20261)
    cases = []
    for wi, (fname, fp) in enumerate(FOOTPRINTS * 2):
        yaws = YAWS + [float(v) for v in rng.uniform(-4, 4, len(GRID) - len(YAWS))]
        boxes = np.array([[cx, cy, EXTENTS[int(rng.integers(len(EXTENTS)))], EXTENTS[int(rng.integers(len(EXTENTS)))], yaw]
                          for (cx, cy), yaw in zip(GRID, [yaws[i] for i in rng.permutation(len(yaws))])])
        hit = collider(orc.lib.orc_collides, fp, boxes)
        poses, rays = [], []
        for m, (cx, cy, bhx, bhy, yaw) in enumerate(boxes):
            for r in range(13):
                th = HEADINGS[int(rng.integers(len(HEADINGS)))] if r % 3 else float(rng.uniform(-7, 7))
                # directions: the box's face normals, its corners, the footprint's face normals, random
                ang = [yaw, yaw + PI / 2, yaw + PI, yaw - PI / 2, yaw + math.atan2(bhy, bhx), yaw + PI - math.atan2(bhy, bhx),
                       th, th + PI / 2, yaw + PI / 4, float(rng.uniform(-PI, PI)), float(rng.uniform(-PI, PI)),
                       yaw + PI + math.atan2(bhy, bhx), float(rng.uniform(-PI, PI))][r]
                ux, uy = math.cos(ang), math.sin(ang)
                if yaw == 0.0 and r < 4:                      # exactly along the world axes
                    ux, uy = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)][r]
                # the footprint's centre starts inside the box (a hit), off the ray through the centres by s
                s = float(rng.uniform(-0.9, 0.9)) * min(bhx, bhy) if r % 2 else 0.0
                tx = cx - (math.cos(th) * fp[0] - math.sin(th) * fp[1]) - s * uy
                ty = cy - (math.sin(th) * fp[0] + math.cos(th) * fp[1]) + s * ux
                t0 = bisect_flip(lambda t: hit(tx + t * ux, ty + t * uy, th))
                first = len(poses)
                poses += [(tx + step(t0, k) * ux, ty + step(t0, k) * uy, th) for k in ULPS]
                rays.append((first, m))
        poses = np.array(poses)
        K = 1 + wi % 8
        centre = np.array([0.0, 0.0, 0.5 * (poses[:, 2].min() + poses[:, 2].max())])
        spread = max(1e3, float(np.ptp(poses[:, 2])))
        params = np.zeros((K, 12))
        for k in range(K):                                   # a mixture whose reach holds every pose by a wide margin
            params[k, :3] = centre + [0.01 * k, -0.02 * k, 0.0]
            params[k, 3:9] = [100.0, 0.0, 100.0, 0.0, 0.0, spread]
        cases.append(dict(name="(a) %s #%d" % (fname, wi), fp=fp, boxes=boxes, params=params, poses=poses, rays=rays,
                          want=np.array([hit(*p) for p in poses]), keeps_all=True))
    return cases


# ---------------------------------------------------------------------------------------------------------------
# (b) exact touches: dyadic numbers, the expected flags written by hand
# ---------------------------------------------------------------------------------------------------------------
def before(v):
    return math.nextafter(v, -math.inf)


def after(v):
    return math.nextafter(v, math.inf)


def touch_cases():
    wide = np.zeros((1, 12))
    wide[0, 3:9] = [100.0, 0.0, 100.0, 0.0, 0.0, 100.0]
    out = []
    # a square footprint of half extent 1/4 at heading 0; walls of half extent 1/4 at x = 1 and y = 1, a square whose corner
    # meets the footprint's at (-1, -2), and a 1/4 x 1/8 box turned by a quarter turn (world half extents 1/8 x 1/4) at x = -1.
    # The predicate's first operation is centre - pose, ROUNDED: from x = 1/2 the next double down is 1/2 - 2^-54, and
    # 1 - (1/2 - 2^-54) ties back to 1/2 -- the same distance, still touching; the first pose whose distance to the wall is
    # another double is 1/2 - 2^-53.  From the far side (x = 3/2) one ulp changes the distance, and misses.
    boxes = [[1.0, 0.0, 0.25, 0.25, 0.0], [0.0, 1.0, 0.25, 0.25, 0.0], [-1.25, -2.25, 0.25, 0.25, 0.0], [-1.0, 0.0, 0.25, 0.125, PI / 2]]
    poses = [((0.5, 0.0, 0.0), True), ((before(0.5), 0.0, 0.0), True), ((0.5 - 2.0 ** -53, 0.0, 0.0), False),   # the wall in x
             ((1.5, 0.0, 0.0), True), ((after(1.5), 0.0, 0.0), False),               # ... from its other side
             ((0.0, 0.5, 0.0), True), ((0.0, before(0.5), 0.0), True), ((0.0, 0.5 - 2.0 ** -53, 0.0), False),   # the wall in y
             ((0.0, 1.5, 0.0), True), ((0.0, after(1.5), 0.0), False),
             ((-0.75, -1.75, 0.0), True), ((after(-0.75), -1.75, 0.0), False), ((-0.75, after(-1.75), 0.0), False),   # corner to corner
             ((-0.625, 0.0, 0.0), True), ((after(-0.625), 0.0, 0.0), False),         # the box at a quarter turn
             ((0.0, 0.0, 0.0), False), ((1.0, 0.0, 0.0), True)]
    out.append(("(b) square footprint", (0.0, 0.0, 0.25, 0.25), boxes, poses))
    # the wall in x met by an OFFSET footprint (its centre half a unit behind the base)
    boxes = [[1.0, 0.0, 0.25, 0.25, 0.0]]
    poses = [((1.0, 0.0, 0.0), True), ((before(1.0), 0.0, 0.0), False), ((2.0, 0.0, 0.0), True), ((after(2.0), 0.0, 0.0), False)]
    out.append(("(b) offset footprint", (-0.5, 0.0, 0.25, 0.25), boxes, poses))
    # a 1/2 x 1/8 footprint at heading pi/2 (the table's sine and cosine there are exactly 1 and -0): 1/8 wide in x
    boxes = [[1.0, 0.0, 0.25, 0.25, 0.0]]
    poses = [((0.625, 0.0, PI / 2), True), ((before(0.625), 0.0, PI / 2), False),
             ((0.0, 0.75, PI / 2), False), ((0.75, 0.75, PI / 2), True), ((0.75, after(0.75), PI / 2), False)]
    out.append(("(b) footprint at a quarter turn", (0.0, 0.0, 0.5, 0.125), boxes, poses))
    return [dict(name=n, fp=fp, boxes=np.array(b), params=wide.copy(), poses=np.array([p for p, _ in ps]),
                 want=np.array([w for _, w in ps]), keeps_all=True) for n, fp, b, ps in out]


# ---------------------------------------------------------------------------------------------------------------
# (c) the edge of a mixture's reach
# ---------------------------------------------------------------------------------------------------------------
def extreme_normals(orc):
    """(z0, z1, z2) of the extreme words: z0, z1 one Box-Muller pair, z2 the first normal of another (pocs_normal3)."""
    out = []
    for wr in (1, 2, 3, 0):
        for wa in (0, 2 ** 30, 2 ** 31, 3 * 2 ** 30, 2 ** 29, 3 * 2 ** 29, 5 * 2 ** 29, 7 * 2 ** 29):
            z0, z1 = orc.normal_pair_w2(wr, wa)
            for wa2 in (0, 2 ** 31):
                out.append((z0, z1, orc.normal_pair_w2(wr, wa2)[0], wr))
    return out


def mixture(orc, comps):
    """comps: (mean3, L00 L10 L11 L20 L21 L22) -> (params K x 12 with the ORACLE's factor of L L^T, covariances)."""
    params, covs = np.zeros((len(comps), 12)), []
    for k, (mean, l) in enumerate(comps):
        L = np.array([[l[0], 0, 0], [l[1], l[2], 0], [l[3], l[4], l[5]]])
        cov = L @ L.T
        ok, Lc = orc.chol3_lower(cov)
        assert ok
        params[k, :3], params[k, 3:9] = mean, Lc
        covs.append(cov)
    return params, covs


# name, footprint, K, mean heading, sigma of the heading, (L20, L21)
MIXTURES = [
    ("K=1 heading 0, end values", (0.0, 0.0, 0.5, 0.05), 1, 0.0, 1e-4, (0.0, 0.0)),
    ("K=3 just below pi/2, offset", (-0.25, 0.3, 0.5, 0.05), 3, PI / 2 - 0.01, 1e-4, (2e-5, -3e-5)),
    ("K=3 across pi/2", (0.0, 0.0, 0.5, 0.05), 3, PI / 2, 0.05, (0.01, -0.02)),
    ("K=8 at 3.1, a peak inside", (0.3, -0.2, 0.5, 0.05), 8, 3.1, 0.05, (-0.01, 0.01)),
    ("K=8 at -3.1, wide", (0.0, 0.0, 0.25, 0.25), 8, -3.1, 0.3, (0.05, 0.05)),
    ("K=3 range over pi: the radius", (0.3, -0.2, 0.25, 0.25), 3, 0.0, 0.6, (-0.1, 0.1)),
    ("K=3 at the peak angle", (0.0, 0.0, 0.5, 0.05), 3, math.atan2(0.05, 0.5), 0.05, (0.0, 0.0)),
    ("K=8 heading tied to x and y", (0.0, 0.0, 0.05, 0.5), 8, 0.0, 1e-4, (0.02, -0.03)),
    ("K=1 at pi/4, offset", (-0.25, 0.3, 0.5, 0.05), 1, PI / 4, 0.05, (0.01, 0.01)),
    ("K=3 at -pi/4", (0.0, 0.0, 0.5, 0.05), 3, -PI / 4, 0.05, (-0.01, -0.01)),
]


def reach_cases(orc):
    rng = np.random.default_rng(20262)
    zs = extreme_normals(orc)
    cases = []
    for name, fp, K, th0, sth, (l20, l21) in MIXTURES:
        comps = []
        for k in range(K):
            sgn = -1.0 if k % 2 else 1.0
            mean = (1.7 * (k % 3) + 0.1 * k, 1.9 * (k // 3) - 0.05 * k, th0 + sth * (0.3 * k - 0.1 * K))
            comps.append((mean, (0.05 + 0.02 * k, sgn * 0.03, 0.06 + 0.01 * k, sgn * l20, -sgn * l21, sth)))
        params, covs = mixture(orc, comps)
        poses, owner_pool = [], []
        for k in range(K):
            ordinary = [orc.normal_pair_w2(int(a), int(b)) + (orc.normal_pair_w2(int(c), int(d))[0], -1)
                        for a, b, c, d in rng.integers(0, 2 ** 32, (24, 4))]
            z = np.array([t[:3] for t in zs + ordinary])
            pts = orc.mvnrnd_tape(params[k, :3], covs[k], z)
            assert pts is not None
            for i, p in enumerate(pts):
                if i < len(zs) and zs[i][3] == 1:
                    owner_pool.append((len(poses), k, zs[i]))
                poses.append(tuple(p))
        poses = np.array(poses)
        # obstacles, one per owning pose: pushed in from outside along a ray until it touches that pose's footprint
        order = [owner_pool[i] for i in rng.permutation(len(owner_pool))]
        owners, obstacles = [], []                       # obstacles: (cx0, cy0, ux, uy, t_hit, hx, hy, yaw)
        single = lambda box: collider(orc.lib.orc_collides, fp, [box])
        for pi_, k, (z0, z1, z2, _) in order:
            if len(owners) == 60:
                break
            x, y, th = poses[pi_]
            sx, sy = (z0 > 0) - (z0 < 0), (z1 > 0) - (z1 < 0)
            dirs = [(float(sx), 0.0)] * (sx != 0) + [(0.0, float(sy))] * (sy != 0)
            if sx and sy:
                dirs.append((sx / math.sqrt(2.0), sy / math.sqrt(2.0)))
            ux, uy = dirs[len(owners) % len(dirs)]
            hx, hy = (float(v) for v in rng.uniform(0.03, 0.3, 2))
            yaw = [0.0, 0.0, PI / 2, float(rng.uniform(-3, 3))][len(owners) % 4]
            cx0 = x + (math.cos(th) * fp[0] - math.sin(th) * fp[1])
            cy0 = y + (math.sin(th) * fp[0] + math.cos(th) * fp[1])
            at = lambda t: [cx0 + t * ux, cy0 + t * uy, hx, hy, yaw]
            t_hit = bisect_flip(lambda t: single(at(t))(x, y, th))
            # no masking: the new obstacle, six ulps inside its flip, touches no other owner, and no obstacle so far touches this pose
            inner = single(at(step(t_hit, -6)))
            if any(inner(*poses[j]) for j, _ in owners):
                continue
            if any(single([o[0] + step(o[4], -6) * o[2], o[1] + step(o[4], -6) * o[3], o[5], o[6], o[7]])(x, y, th) for o in obstacles):
                continue
            owners.append((pi_, len(obstacles)))
            obstacles.append((cx0, cy0, ux, uy, t_hit, hx, hy, yaw))
        for off in C_OFFSETS:
            boxes = np.array([[o[0] + step(o[4], off) * o[2], o[1] + step(o[4], off) * o[3], o[5], o[6], o[7]] for o in obstacles])
            hit = collider(orc.lib.orc_collides, fp, boxes)
            cases.append(dict(name="(c) %s, obstacles at %+d ulps" % (name, off), fp=fp, boxes=boxes, params=params, poses=poses,
                              owners=owners, offset=off, mixture=name, want=np.array([hit(*p) for p in poses]), keeps_all=False))
    return cases


# ---------------------------------------------------------------------------------------------------------------
# (d) far obstacles
# ---------------------------------------------------------------------------------------------------------------
def far_cases(orc):
    rng = np.random.default_rng(20263)
    fp = (0.0, 0.0, 0.3, 0.2)
    comps = [((0.0, 0.0, 0.2), (0.05, 0.01, 0.05, 0.0, 0.0, 0.05)), ((1.5, 0.5, 0.3), (0.05, -0.01, 0.05, 0.0, 0.0, 0.05)),
             ((0.5, 2.0, 0.1), (0.05, 0.0, 0.05, 0.01, 0.0, 0.05))]
    params, covs = mixture(orc, comps)
    zs = np.array([t[:3] for t in extreme_normals(orc)])
    poses = np.concatenate([orc.mvnrnd_tape(params[k, :3], covs[k], zs) for k in range(3)])
    # near: centred inside the bounding box of the means; far: 40 away from it, where reach (0.4) + footprint radius (0.37)
    # + the largest box radius (2.2) is 3
    near = [[float(rng.uniform(0.0, 1.5)), float(rng.uniform(0.0, 2.0)), float(rng.uniform(0.05, 0.2)), float(rng.uniform(0.05, 0.2)),
             float(rng.uniform(-3, 3))] for _ in range(9)]
    far = [[0.75 + 40.0 * math.cos(a), 1.0 + 40.0 * math.sin(a), float(rng.uniform(0.05, 1.5)), float(rng.uniform(0.05, 1.5)),
            float(rng.uniform(-3, 3))] for a in np.linspace(0.0, 2 * PI, 55, endpoint=False)]
    order = rng.permutation(64)
    boxes = np.array(near + far)[order]
    worlds = [("M = 64", boxes, 9), ("M = 1 in reach", np.array(near[:1]), 1), ("M = 1 out of reach", np.array(far[:1]), 0),
              ("M = 0", np.zeros((0, 5)), 0)]
    cases = []
    for name, b, nkeep in worlds:
        hit = collider(orc.lib.orc_collides, fp, b)
        cases.append(dict(name="(d) " + name, fp=fp, boxes=b, params=params, poses=poses, nkeep=nkeep,
                          want=np.array([hit(*p) for p in poses]), keeps_all=False))
    return cases


@pytest.fixture(scope="module")
def cases(orc):
    """Every input of this file with the oracle's flags, built once."""
    return dict(a=grazing_cases(orc), b=touch_cases(), c=reach_cases(orc), d=far_cases(orc))


# ---------------------------------------------------------------------------------------------------------------
# CPU leg
# ---------------------------------------------------------------------------------------------------------------
def test_exact_touches_hit_and_one_ulp_further_misses(cases, orc, hh):
    """(b): the flags written down by hand, from the oracle and from the host build of the product's predicate."""
    n = 0
    for c in cases["b"]:
        for fn in (orc.lib.orc_collides, hh.hh_collides):
            hit = collider(fn, c["fp"], c["boxes"])
            got = np.array([hit(*p) for p in c["poses"]])
            assert np.array_equal(got, c["want"]), (c["name"], fn, c["poses"][got != c["want"]])
        n += len(c["poses"])
    assert n >= 24


def test_host_predicate_equals_oracle_on_grazing_and_reach_edge_poses(cases, hh):
    """(a), (c), (d): hh_collides == orc.collides on every pose, nothing skipped."""
    poses = hits = 0
    for c in cases["a"] + cases["c"] + cases["d"]:
        hit = collider(hh.hh_collides, c["fp"], c["boxes"])
        got = np.array([hit(*p) for p in c["poses"]])
        bad = np.flatnonzero(got != c["want"])
        assert bad.size == 0, (c["name"], c["fp"], [(tuple(c["poses"][i]), bool(c["want"][i])) for i in bad[:5]])
        poses += len(got)
        hits += int(got.sum())
    assert poses > 30000 and hits > 5000 and poses - hits > 5000, (poses, hits)


def test_generated_inputs_are_not_vacuous(cases):
    """The bisected rays straddle the boundary -- the flags at -6 and +6 ulps differ (a flag that flips twice within
    twelve ulps is the one legitimate exception: at least 95 %) -- and both outcomes are well represented."""
    rays = flips = 0
    for c in cases["a"]:
        for first, _ in c["rays"]:
            w = c["want"][first:first + len(ULPS)]
            assert w[ULPS.index(0)] and not w[ULPS.index(1)], (c["name"], first)       # the bisection's own two poses
            rays += 1
            flips += bool(w[ULPS.index(-6)] != w[ULPS.index(6)])
    hits = sum(int(c["want"].sum()) for c in cases["a"])
    poses = sum(len(c["want"]) for c in cases["a"])
    assert rays >= 1500 and flips >= 0.95 * rays and hits > 0.3 * poses and poses - hits > 0.3 * poses, (rays, flips, poses, hits)
    # (c): per mixture, the owning poses' flags in the world of obstacles at -6 ulps and in the world at +6
    by_mix = {}
    for c in cases["c"]:
        by_mix.setdefault(c["mixture"], {})[c["offset"]] = c
    owners = flips_c = 0
    for name, w in by_mix.items():
        own = [p for p, _ in w[-6]["owners"]]
        # (eight outward directions per component; the two poses that differ in the sign of the heading's normal lie at
        # nearly one place and share an obstacle where the heading is narrow: at least five a component)
        assert len(own) >= 5 * len(w[-6]["params"]), (name, len(own))
        assert all(w[0]["want"][p] for p in own), name
        owners += len(own)
        flips_c += sum(bool(w[-6]["want"][p] != w[6]["want"][p]) for p in own)
        free = sum(int(not v) for v in w[6]["want"])
        assert free > 0.3 * len(w[6]["want"]), (name, free)
    assert len(by_mix) == len(MIXTURES) and flips_c >= 0.95 * owners, (owners, flips_c)


# ---------------------------------------------------------------------------------------------------------------
# GPU leg
# ---------------------------------------------------------------------------------------------------------------
def table_records(hh, fp, boxes):
    """The obstacle table as the host prepares it (pocs_prepare_obstacle)."""
    fp_a = (C.c_double * 4)(*fp)
    rec = np.zeros((len(boxes), 8))
    for m, b in enumerate(np.ascontiguousarray(boxes, dtype=np.float64)):
        hh.hh_prepare_obstacle(b.ctypes.data_as(C.POINTER(C.c_double)), fp_a, rec[m].ctypes.data_as(C.POINTER(C.c_double)))
    return rec


def probe_and_check(ctx, orc, hh, c):
    """One launch: the three device flags == the oracle on every pose; the kept records are the table's, in table order,
    with a broad phase no wider than the table's and no narrower than box + footprint can need; nothing a probed pose
    hits was dropped.  Returns the indices of the kept boxes."""
    fp, boxes, poses = c["fp"], c["boxes"], c["poses"]
    ctx.set_env(dict(footprint=fp, boxes=boxes))
    full, pair, eager, kept = ctx.probe_device_collide(c["params"], poses)
    want = c["want"].astype(np.int32)
    for what, got in (("pocs_pose_collides, full table", full), ("pocs_pair_collides<false>, culled table", pair),
                      ("pocs_pair_collides<true>, culled table", eager)):
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (c["name"], what, len(bad), [(int(i), tuple(poses[i]), int(got[i]), int(want[i])) for i in bad[:5]])
    table = table_records(hh, fp, boxes)
    idx, m = [], 0
    for r in kept:                                       # order-preserving compaction
        while m < len(table) and not np.array_equal(table[m, :6], r[:6]):
            m += 1
        assert m < len(table), (c["name"], "a kept record is not the table's, or out of order", r)
        idx.append(m)
        m += 1
    for r, m in zip(kept, idx):
        t = table[m]
        assert r[6] <= t[6] and r[7] <= t[7], (c["name"], m, r, t)
        wx = t[4] * abs(t[2]) + t[5] * abs(t[3])
        wy = t[4] * abs(t[3]) + t[5] * abs(t[2])
        assert r[6] >= wx + min(fp[2], fp[3]) and r[7] >= wy + min(fp[2], fp[3]), (c["name"], m, r, t)
    if c["keeps_all"]:
        assert idx == list(range(len(boxes))), (c["name"], idx)
    # every box a probed pose hits is among the kept (a centre distance beyond the two radii cannot hit: not asked)
    rr = math.hypot(fp[2], fp[3]) + math.hypot(fp[0], fp[1])
    for m in sorted(set(range(len(boxes))) - set(idx)):
        b = boxes[m]
        close = np.flatnonzero(np.hypot(poses[:, 0] - b[0], poses[:, 1] - b[1]) <= 1.001 * (rr + math.hypot(b[2], b[3])) + 1e-9)
        hit = collider(orc.lib.orc_collides, fp, [b])
        assert not any(hit(*poses[i]) for i in close), (c["name"], "a dropped box is hit by a probed pose", m, b)
    return idx


@pytest.mark.gpu
def test_device_predicate_on_grazing_poses_and_exact_touches(pocs, cases, orc, hh):
    """(a), (b): flag_full == flag_pair == flag_pair_eager == the oracle (for (b): == the flags written by hand) on
    every pose, under a mixture whose reach holds them all: every box is kept."""
    with pocs.Context(0) as ctx:
        for c in cases["a"] + cases["b"]:
            probe_and_check(ctx, orc, hh, c)


@pytest.mark.gpu
def test_device_cull_at_the_edge_of_the_mixture_reach(pocs, cases, orc, hh):
    """(c): the poses a mixture can draw at most, against obstacles that touch or just miss them: the culled table gives
    the oracle's flags, and the obstacle of every owning pose that it hits is kept."""
    with pocs.Context(0) as ctx:
        for c in cases["c"]:
            idx = probe_and_check(ctx, orc, hh, c)
            if c["offset"] <= 0:
                lost = [(p, o) for p, o in c["owners"] if o not in idx]
                assert not lost, (c["name"], "touching obstacles dropped", lost[:5])


@pytest.mark.gpu
def test_device_cull_drops_far_obstacles_and_keeps_table_order(pocs, cases, orc, hh):
    """(d): of 64 boxes the nine within the mixture's bounding box are kept, in table order, the 55 far ones dropped; one
    box in reach is kept, one out of reach dropped, an empty world keeps nothing."""
    with pocs.Context(0) as ctx:
        for c in cases["d"]:
            idx = probe_and_check(ctx, orc, hh, c)
            assert len(idx) == c["nkeep"], (c["name"], idx)
            if len(c["boxes"]) == 64:
                assert idx == [m for m, b in enumerate(c["boxes"]) if math.hypot(b[0] - 0.75, b[1] - 1.0) < 10.0], idx


@pytest.mark.gpu
def test_probe_refusals_leave_the_context_usable(pocs, cases, orc, hh):
    """Null-like and non-finite inputs are refused before anything reaches the device (a NaN heading has no sector),
    with the codes the setters use; after each refusal the context still answers a valid probe."""
    c = cases["b"][0]
    nan_pose, inf_mean = c["poses"].copy(), c["params"].copy()
    nan_pose[3, 2] = float("nan")
    inf_mean[0, 0] = float("inf")
    with pocs.Context(0) as ctx:
        with pytest.raises(pocs.PocsError) as e:             # no collision world yet: as the run calls answer (test_error_behaviour)
            ctx.probe_device_collide(c["params"], c["poses"])
        assert e.value.code == -3 and "collision world" in str(e.value)
        probe_and_check(ctx, orc, hh, c)
        for params, poses in ((c["params"], nan_pose), (inf_mean, c["poses"]), (np.zeros((0, 12)), c["poses"]),
                              (np.tile(c["params"], (9, 1)), c["poses"]), (c["params"], np.zeros((0, 3)))):
            with pytest.raises(pocs.PocsError) as e:
                ctx.probe_device_collide(params, poses)
            assert e.value.code == -1, (e.value, params.shape, poses.shape)
            probe_and_check(ctx, orc, hh, c)
