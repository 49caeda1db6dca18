"""Plan / collision-world I/O (text formats written by tools/make_plan_fixture.py).

Reference counterparts: MCSimulation.py:176-198 (loads trajectory.dat / odometry.dat and sends
them by component), gaussprop.py:166-172 (getPathOdometry = inverseOdometry over consecutive
waypoints, MCSimulator.h:434-449) and the obstacle boxes of pr2test2.env.xml.
"""
import math
from pathlib import Path

import numpy as np

DATA = Path(__file__).resolve().parent / "data"

# Parameters of every published run (gaussprop.py:36,39,45-46,56; MCSimulation.py:164,204-205).
DEFAULTS = dict(
    alphas=[0.00025 ** 2, 0.0025 ** 2, 0.0025 ** 2, 0.0025 ** 2],
    Q=0.2 ** 2,
    landmarks=[[3, -3, 0, 0, -3, 3, -3, 3], [0, 0, 2, -2, 2, 2, -2, -2]],
    cov0=[[0.001, 0, 0], [0, 0.001, 0], [0, 0, 0.001]],
    num_particles=10000,
    num_gaussians=3,
)


def load_plan(path=None):
    """Returns dict(traj: W x 3 [x y theta], odom: (W-1) x 3 [drot1 dtrans drot2])."""
    path = Path(path) if path else DATA / "pr2test2_plan.txt"
    rows = [ln.split() for ln in path.read_text().splitlines() if ln.strip() and not ln.startswith("#")]
    W = int(rows[0][0])
    vals = np.array([[float(v) for v in r] for r in rows[1:]], dtype=np.float64)
    if vals.shape != (2 * W - 1, 3):
        raise ValueError("plan file %s: expected %d rows of 3, got %s" % (path, 2 * W - 1, vals.shape))
    return dict(traj=vals[:W].copy(), odom=vals[W:].copy())


def load_env(path=None):
    """Returns dict(footprint: [dx dy hx hy], boxes: M x 5 [cx cy hx hy yaw])."""
    path = Path(path) if path else DATA / "pr2test2_env.txt"
    fp, boxes = [0.0, 0.0, 0.334, 0.334], []
    for ln in path.read_text().splitlines():
        t = ln.split()
        if not t or t[0].startswith("#"):
            continue
        if t[0] == "footprint":
            fp = [float(v) for v in t[1:5]]
        elif t[0] == "box":
            boxes.append([float(v) for v in t[1:6]])
        else:
            raise ValueError("env file %s: unknown record %r" % (path, t[0]))
    return dict(footprint=fp, boxes=np.array(boxes, dtype=np.float64).reshape(-1, 5))


def wrap_angle(a):
    """angleWrap, MCSimulator.h:56-65 (while loops into [0, 2 pi], 2 pi itself kept)."""
    while a < 0:
        a += 2 * math.pi
    while a > 2 * math.pi:
        a -= 2 * math.pi
    return a


def inverse_odometry(p1, p2):
    """inverseOdometry, MCSimulator.h:434-449."""
    r1 = wrap_angle(math.atan2(p2[1] - p1[1], p2[0] - p1[0]) - p1[2])
    tr = math.sqrt((p2[0] - p1[0]) ** 2 + (p2[1] - p1[1]) ** 2)
    r2 = wrap_angle(p2[2] - p1[2] - r1)
    return [r1, tr, r2]


def path_odometry(traj):
    """getPathOdometry, gaussprop.py:166-172: odometry between consecutive waypoints."""
    traj = np.asarray(traj, dtype=np.float64)
    return np.array([inverse_odometry(traj[i], traj[i + 1]) for i in range(len(traj) - 1)])


def resample_plan(plan, W):
    """W-waypoint plan on the same polyline: x, y piecewise linear in the
    index parameter s = j (W0-1)/(W-1); theta piecewise constant from the segment's start
    waypoint; odometry regenerated with inverse_odometry."""
    t0 = np.asarray(plan["traj"], dtype=np.float64)
    W0 = len(t0)
    out = np.zeros((W, 3))
    for j in range(W):
        s = j * (W0 - 1) / (W - 1) if W > 1 else 0.0
        i = min(int(math.floor(s)), W0 - 2) if W0 > 1 else 0
        f = s - i
        if W0 > 1:
            out[j, 0] = t0[i, 0] + f * (t0[i + 1, 0] - t0[i, 0])
            out[j, 1] = t0[i, 1] + f * (t0[i + 1, 1] - t0[i, 1])
            out[j, 2] = t0[i, 2] if f < 1.0 else t0[i + 1, 2]
        else:
            out[j] = t0[0]
    return dict(traj=out, odom=path_odometry(out))


MAX_TREE_NODES = 4096


def check_tree(parent, poses, odoms):
    """A tree of plans as pocs_set_plan_tree takes it -> (parent int32[T], poses float64 T x 3, odoms float64 T x 3), or
    ValueError: one root (parent[0] = -1), every other node after its parent (0 <= parent[n] < n), 1 <= T <= 4096."""
    parent = np.ascontiguousarray(parent, dtype=np.int32)
    poses = np.ascontiguousarray(poses, dtype=np.float64)
    odoms = np.ascontiguousarray(odoms, dtype=np.float64)
    T = len(parent)
    if parent.ndim != 1 or not 1 <= T <= MAX_TREE_NODES:
        raise ValueError("a tree has between 1 and %d nodes, got %s" % (MAX_TREE_NODES, parent.shape))
    if poses.shape != (T, 3) or odoms.shape != (T, 3):
        raise ValueError("poses and odoms are T x 3 with T = %d, got %s and %s" % (T, poses.shape, odoms.shape))
    if parent[0] != -1:
        raise ValueError("node 0 is the root: parent[0] must be -1, got %d" % parent[0])
    for n in range(1, T):
        if not 0 <= parent[n] < n:
            raise ValueError("parent[%d] = %d: one root, and every other node comes after its parent" % (n, parent[n]))
    return parent, poses, odoms


def tree_from_plans(plans):
    """Merges the common prefixes of plans ({"traj": W x 3, "odom": (W-1) x 3} each) that start at the same pose into a
    tree -> (parent, poses, odoms, leaf_of_plan): node arrays as Context.set_plan_tree takes them (nodes in the order the
    plans first reach them, so parent[n] < n) and, per plan, the node its last waypoint became.  Two plans share a node only
    where every pose and every control up to it is equal as float64 BITS (0.0 and -0.0 differ, a NaN equals itself)."""
    plans = list(plans)
    if not plans:
        raise ValueError("no plans")
    parent, poses, odoms, leaf = [], [], [], []
    child = {}                                   # (parent node, bits of the control and the pose) -> node
    for i, pl in enumerate(plans):
        t = np.ascontiguousarray(pl["traj"], dtype=np.float64)
        o = np.ascontiguousarray(pl["odom"], dtype=np.float64).reshape(-1, 3)
        if t.ndim != 2 or t.shape[1] != 3 or t.shape[0] < 1 or o.shape != (t.shape[0] - 1, 3):
            raise ValueError("plan %d: trajectory %s / odometry %s, W x 3 and (W - 1) x 3 expected" % (i, t.shape, o.shape))
        at = -1
        for w in range(t.shape[0]):
            key = (at, o[w - 1].tobytes() if w else b"", t[w].tobytes())
            n = child.get(key)
            if n is None:
                if w == 0 and parent:
                    raise ValueError("plan %d starts at another pose than plan 0: a tree has one root" % i)
                n = len(parent)
                if n >= MAX_TREE_NODES:
                    raise ValueError("the plans make a tree of more than %d nodes" % MAX_TREE_NODES)
                child[key] = n
                parent.append(at)
                poses.append(t[w].copy())
                odoms.append(o[w - 1].copy() if w else np.zeros(3))
            at = n
        leaf.append(at)
    return (np.array(parent, dtype=np.int32), np.array(poses, dtype=np.float64).reshape(-1, 3),
            np.array(odoms, dtype=np.float64).reshape(-1, 3), np.array(leaf, dtype=np.int32))


def tree_path(parent, poses, odoms, n):
    """The path root -> n of a tree as a plan dict(traj: W x 3, odom: (W-1) x 3), W = depth(n) + 1."""
    parent, poses, odoms = check_tree(parent, poses, odoms)
    if not 0 <= n < len(parent):
        raise ValueError("node %d outside the tree (0..%d)" % (n, len(parent) - 1))
    path = []
    while n >= 0:
        path.append(n)
        n = int(parent[n])
    path.reverse()
    return dict(traj=poses[path].copy(), odom=odoms[path[1:]].copy().reshape(-1, 3))


def moving_boxes(boxes0, velocity, S):
    """An obstacle schedule (Context.set_obstacle_schedule) from boxes that move at constant velocity: boxes0 M x 5
    (cx, cy, half_x, half_y, yaw), velocity M x 3 = (vx, vy, omega) per waypoint.  Returns S x M x 5; step s of box m is
    (cx + s * vx, cy + s * vy, half_x, half_y, yaw + s * omega), each one multiplication and one addition in IEEE double."""
    b = np.asarray(boxes0, dtype=np.float64).reshape(-1, 5)
    v = np.asarray(velocity, dtype=np.float64).reshape(-1, 3)
    S = int(S)
    if v.shape[0] != b.shape[0]:
        raise ValueError("velocity of %d boxes for %d boxes" % (v.shape[0], b.shape[0]))
    if S < 1:
        raise ValueError("a schedule has at least one step, got %d" % S)
    out = np.empty((S, b.shape[0], 5))
    for s in range(S):
        out[s] = b
        out[s, :, 0] = b[:, 0] + float(s) * v[:, 0]
        out[s, :, 1] = b[:, 1] + float(s) * v[:, 1]
        out[s, :, 4] = b[:, 4] + float(s) * v[:, 2]
    return out


def moving_discs(tracks, r):
    """A disc schedule (Context.set_discs) from per-waypoint centres, the counterpart of moving_boxes: tracks of shape (S, D, 2) --
    tracks[s, d] the centre of disc d at waypoint s, as a predictor hands it over -- or (S, 2) for a single disc; r a radius for
    all discs or one per disc (D).  Returns S x D x 3 = (cx, cy, r): the values as they are, no arithmetic.  ValueError for a
    shape that is neither, an empty track, or a radius that is not positive and finite."""
    t = np.asarray(tracks, dtype=np.float64)
    if t.ndim == 2 and t.shape[1] == 2:
        t = t.reshape(t.shape[0], 1, 2)
    if t.ndim != 3 or t.shape[2] != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError("tracks of shape %s, (S, D, 2) with S, D >= 1 expected" % (t.shape,))
    rr = np.asarray(r, dtype=np.float64).ravel()
    if rr.size == 1:
        rr = np.repeat(rr, t.shape[1])
    if rr.size != t.shape[1]:
        raise ValueError("%d radii for %d discs" % (rr.size, t.shape[1]))
    if not (np.all(np.isfinite(rr)) and np.all(rr > 0.0)):
        raise ValueError("a disc's radius is positive and finite")
    out = np.empty((t.shape[0], t.shape[1], 3))
    out[:, :, :2] = t
    out[:, :, 2] = rr[None, :]
    return out


def prediction_covariances(sigma0, rate, S, D):
    """Disc covariances (Context.set_disc_covariances) of a constant-velocity predictor's fan: isotropic, standard deviation
    sigma0 + rate * s at disc step s, for S steps of D discs.  Returns S x D x 3 = (sxx, sxy, syy) with (sigma0 + rate s)^2 on the
    diagonal and sxy = 0.  ValueError for S or D below 1 or a standard deviation that is negative or not finite."""
    S, D = int(S), int(D)
    if S < 1 or D < 1:
        raise ValueError("S and D are at least 1")
    sig = float(sigma0) + float(rate) * np.arange(S, dtype=np.float64)
    if not (np.all(np.isfinite(sig)) and np.all(sig >= 0.0)):
        raise ValueError("a standard deviation is non-negative and finite")
    out = np.zeros((S, D, 3))
    out[:, :, 0] = (sig * sig)[:, None]
    out[:, :, 2] = (sig * sig)[:, None]
    return out


def prediction_modes(agents, radius):
    """A multi-modal prediction as discs with hypotheses (Context.set_discs, Context.set_disc_hypotheses).  `agents`: a list of agents,
    each a list of (weight, track) alternatives with track of shape S x 2 (the same S everywhere); `radius`: one radius, or one per
    agent.  Returns (discs S x D x 3, group int32[D], weight float64[D]) with D the number of alternatives of all agents: agent a's
    alternatives are the discs of one group, named by the index of its first disc.  ValueError for no agent, an agent without
    alternatives, ragged S, a weight outside (0, 1], a group sum above 1 and any value that is not finite."""
    agents = [list(a) for a in agents]
    if not agents or any(not a for a in agents):
        raise ValueError("at least one agent, each with at least one (weight, track) alternative")
    radii = np.broadcast_to(np.asarray(radius, dtype=np.float64), (len(agents),)) if np.ndim(radius) <= 1 else None
    if radii is None or not (np.all(np.isfinite(radii)) and np.all(radii > 0.0)):
        raise ValueError("a radius is finite and positive, one for all agents or one per agent")
    cols, group, weight, S = [], [], [], None
    for a, alts in enumerate(agents):
        g, total = len(cols), 0.0
        for w, track in alts:
            w, t = float(w), np.asarray(track, dtype=np.float64)
            if t.ndim != 2 or t.shape[1] != 2 or t.shape[0] < 1:
                raise ValueError("a track is S x 2")
            S = t.shape[0] if S is None else S
            if t.shape[0] != S:
                raise ValueError("ragged tracks: %d steps beside %d" % (t.shape[0], S))
            if not (np.isfinite(w) and 0.0 < w <= 1.0):
                raise ValueError("a weight lies in (0, 1]")
            if not np.all(np.isfinite(t)):
                raise ValueError("a track is finite")
            total += w
            cols.append(np.column_stack([t, np.full(S, radii[a])]))
            group.append(g)
            weight.append(w)
        if total > 1.0:
            raise ValueError("the weights of agent %d sum to %r, more than 1" % (a, total))
    return np.stack(cols, axis=1), np.array(group, dtype=np.int32), np.array(weight, dtype=np.float64)


def goal_region(plan, half_x, half_y):
    """The goal tolerance of a plan as a watched region (Context.set_regions): the box (cx, cy, half_x, half_y, yaw) centred at
    the plan's last waypoint and turned to its heading.  `plan` is a dict with `traj` (W x 3) or the W x 3 array itself.
    ValueError for an empty plan or a half extent that is not positive and finite."""
    traj = np.asarray(plan["traj"] if isinstance(plan, dict) else plan, dtype=np.float64).reshape(-1, 3)
    hx, hy = float(half_x), float(half_y)
    if traj.shape[0] < 1:
        raise ValueError("a plan has at least one waypoint")
    if not (math.isfinite(hx) and math.isfinite(hy) and hx > 0.0 and hy > 0.0):
        raise ValueError("half extents must be positive and finite, got %r, %r" % (half_x, half_y))
    x, y, th = traj[-1]
    return np.array([x, y, hx, hy, th], dtype=np.float64)


MAX_WORLD_BOXES = 4096


def grid_boxes(occupancy, cell, origin=(0.0, 0.0)):
    """A 2-D boolean occupancy grid -> boxes M x 5 (cx, cy, half_x, half_y, yaw = 0) as Context.set_world takes them: one box per
    maximal horizontal run of occupied cells.  occupancy[r][c] is the cell [origin_x + c * cell, origin_x + (c + 1) * cell] x
    [origin_y + r * cell, origin_y + (r + 1) * cell]; the boxes come row by row, left to right.  ValueError for a grid that is not
    2-D, a cell size that is not positive, or more than 4096 boxes."""
    occ = np.asarray(occupancy).astype(bool)
    cell = float(cell)
    if occ.ndim != 2:
        raise ValueError("an occupancy grid is 2-D, got shape %s" % (occ.shape,))
    if not cell > 0.0:
        raise ValueError("the cell size must be positive, got %r" % cell)
    x0, y0 = float(origin[0]), float(origin[1])
    boxes = []
    for r in range(occ.shape[0]):
        c = 0
        while c < occ.shape[1]:
            if not occ[r, c]:
                c += 1
                continue
            c1 = c
            while c1 + 1 < occ.shape[1] and occ[r, c1 + 1]:
                c1 += 1
            n = c1 - c + 1
            boxes.append([x0 + cell * (c + 0.5 * n), y0 + cell * (r + 0.5), 0.5 * cell * n, 0.5 * cell, 0.0])
            c = c1 + 1
    if len(boxes) > MAX_WORLD_BOXES:
        raise ValueError("the grid makes %d boxes, a world holds at most %d" % (len(boxes), MAX_WORLD_BOXES))
    return np.array(boxes, dtype=np.float64).reshape(-1, 5)
