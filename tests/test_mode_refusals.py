"""What a context may be asked to do while it is in a mode (csrc/pocs_modes.hpp): a literal table of
(active state, call, expected code), read from the library as it stood before the combination rules moved into one table.
After every refusal the context keeps what it had, and at the end of each context a plain GMM run from the same seed gives the
bits of the run made before the refusals.  No sampling kernel is launched besides those runs (and pocs_gmm_begin's uploads)."""
import ctypes as C

import numpy as np
import pytest

from test_large_world import clutter
from test_plan_risk_bound import prefix

pytestmark = pytest.mark.gpu
K, N, SEED = 3, 1000, 21
OK, E_ARG, E_ORDER, E_STATE = 0, -1, -2, -3


class Things:
    """The arguments the calls below take, made once per test from the bundled plan and room."""

    def __init__(self, pocs, plan, env):
        self.pocs, self.plan, self.env = pocs, plan, env
        self.plans = [plan, prefix(plan, 30)]
        traj, odom = np.asarray(plan["traj"], np.float64), np.asarray(plan["odom"], np.float64)
        self.tree = ([-1, 0], traj[:2].copy(), np.vstack([np.zeros(3), odom[0]]))
        self.w100, self.w64 = clutter(env, 100), clutter(env, 64)
        self.w100_nan = self.w100.copy()
        self.w100_nan[37, 1] = np.nan
        self.ptr = None                                   # a device pointer: the context's own moments (set by `fresh`)


CALLS = {
    "set_path_length": lambda c, x: c._chk(c.lib.pocs_set_path_length(c.h, 56)),
    "set_trajectory": lambda c, x: c._chk(c.lib.pocs_set_trajectory(c.h, np.zeros(168).ctypes.data_as(C.POINTER(C.c_double)), 56)),
    "set_odometry": lambda c, x: c._chk(c.lib.pocs_set_odometry(c.h, np.zeros(165).ctypes.data_as(C.POINTER(C.c_double)), 55)),
    "set_batch": lambda c, x: c.set_batch(2),
    "select_batch_run": lambda c, x: c.select_batch_run(0),
    "set_plans": lambda c, x: c.set_plans(x.plans),
    "set_plans(0)": lambda c, x: c.clear_plans(),
    "set_plans(300)": lambda c, x: c._chk(c.lib.pocs_set_plans(c.h, 300, None, None, None)),
    "set_plan_tree": lambda c, x: c.set_plan_tree(*x.tree),
    "set_plan_tree(0)": lambda c, x: c.clear_plan_tree(),
    "set_plan_risk_bound": lambda c, x: c.set_plan_risk_bound(0.5),
    "set_shard": lambda c, x: c.set_shard(0, 500),
    "set_shard(-1,-1)": lambda c, x: c.set_shard(-1, -1),
    "xchg_create": lambda c, x: c.xchg_create(1, 0),
    "xchg_connect": lambda c, x: c.xchg_connect([b"\0" * 64]),
    "gmm_begin": lambda c, x: c.gmm_begin(),
    "set_world(100)": lambda c, x: c.set_world(x.w100),
    "set_world(64)": lambda c, x: c.set_world(x.w64),
    "set_world(100, one NaN)": lambda c, x: c.set_world(x.w100_nan),
    "bind_moments": lambda c, x: c.gmm_bind_moments(x.ptr, 56 * K * 11),
    "bind_moments(null)": lambda c, x: c.gmm_bind_moments(None, 0),
    "OBSTACLE_COUNTS": lambda c, x: c.set_option(x.pocs.OPT_OBSTACLE_COUNTS, 1),
    "MC_FUSED": lambda c, x: c.set_option(x.pocs.OPT_MC_FUSED, 1),
    "probe_device_collide": lambda c, x: c.probe_device_collide(np.zeros((1, 12)), np.zeros((2, 3))),
    "addObstacle": lambda c, x: c.send_command("addObstacle 0 0 1 1 0"),
}


def state(c):
    """What a refusal must leave as it was: the path length, the world, and what pocs_get_tree_probabilities answers."""
    try:
        tree = tuple(c.tree_probabilities())
    except Exception as e:                                # (PocsError: its code is the answer)
        tree = ("refused", e.code)
    return (c.path_length(), c.world_boxes(), c.world_steps(), tree)


def check(c, x, rows):
    """Makes the calls of `rows`; returns the texts of the refusals."""
    texts = []
    for name, want in rows:
        before = state(c)
        if want == OK:
            CALLS[name](c, x)
            continue
        with pytest.raises(x.pocs.PocsError) as e:
            CALLS[name](c, x)
        print("%-28s %d  %s" % (name, e.value.code, e.value))
        assert e.value.code == want, (name, str(e.value))
        assert state(c) == before, name
        texts.append(str(e.value))
    return texts


def fresh(x, c):
    """Configured on the bundled plan and room; a run has been made, so the context owns a moments buffer."""
    c.configure(x.plan, x.env, K=K, N=N, seed=SEED)
    c.run_gmm_estimation()
    x.ptr = c.gmm_moments_ptr(0)
    assert x.ptr
    c.set_seed(SEED)


def run_again(c, p0):
    c.set_seed(SEED)
    p = c.run_gmm_estimation()
    assert p == p0
    return p


SINGLE = ["set_path_length", "set_trajectory", "set_odometry", "set_batch"]


def test_plans_set(pocs, plan, env):
    x = Things(pocs, plan, env)
    with pocs.Context(0) as c:
        fresh(x, c)
        c.set_plans(x.plans)
        p0 = c.run_gmm_estimation()
        check(c, x, [(n, E_ORDER) for n in SINGLE + ["set_plan_tree"]] +
              [(n, E_STATE) for n in ("set_shard", "xchg_create", "gmm_begin")] + [("set_shard(-1,-1)", OK), ("set_plan_tree(0)", OK)])
        assert c.path_length() == 56 and len(c.batch_probabilities()) == 2      # (the plans are still set)
        run_again(c, p0)


def test_tree_set(pocs, plan, env):
    x = Things(pocs, plan, env)
    with pocs.Context(0) as c:
        fresh(x, c)
        c.set_plan_tree(*x.tree)
        p0 = c.run_gmm_estimation()
        t0 = c.tree_probabilities().copy()
        check(c, x, [(n, E_ORDER) for n in SINGLE + ["set_plans", "select_batch_run"]] +
              [(n, E_STATE) for n in ("set_shard", "xchg_create", "gmm_begin", "set_world(100)")] +
              [("set_plans(300)", E_ARG), ("set_world(100, one NaN)", E_ARG), ("set_plans(0)", OK)])
        assert np.array_equal(c.tree_probabilities(), t0)                       # set_plans(0) left the tree and its results
        check(c, x, [("set_world(64)", OK)])
        assert c.world_boxes() == 64 and c.path_length() == 1
        with pytest.raises(pocs.PocsError) as e:                                # (the tree is still set)
            c.set_batch(2)
        assert e.value.code == E_ORDER and "tree" in str(e.value)
        c.set_env(env)
        run_again(c, p0)
        assert np.array_equal(c.tree_probabilities(), t0)


def test_shard_set(pocs, plan, env):
    x = Things(pocs, plan, env)
    with pocs.Context(0) as c:
        fresh(x, c)
        c.set_shard(0, 500)
        p0 = c.run_gmm_estimation()
        check(c, x, [(n, E_STATE) for n in ("set_plans", "set_plan_tree", "set_world(100)")])
        run_again(c, p0)


def test_exchange(pocs, plan, env):
    x = Things(pocs, plan, env)
    with pocs.Context(0) as c:                                                  # connected: a world of one
        fresh(x, c)
        p0 = c.run_gmm_estimation()
        c.xchg_connect([c.xchg_create(1, 0)])
        check(c, x, [(n, E_STATE) for n in ("set_plans", "set_plan_tree", "set_world(100)")])
        run_again(c, p0)
    with pocs.Context(0) as c:                                                  # created only
        fresh(x, c)
        p0 = c.run_gmm_estimation()
        c.xchg_create(1, 0)
        texts = check(c, x, [("set_world(100)", E_STATE), ("set_plans", OK), ("xchg_connect", E_STATE)])
        assert "pocs_xchg_connect" in texts[-1]
        c.clear_plans()
        run_again(c, p0)


def test_moments_bound(pocs, plan, env):
    x = Things(pocs, plan, env)
    with pocs.Context(0) as c:
        fresh(x, c)
        p0 = c.run_gmm_estimation()
        c.gmm_bind_moments(x.ptr, 56 * K * 11)
        check(c, x, [("set_world(100)", E_STATE), ("bind_moments(null)", OK)])
        run_again(c, p0)


def test_large_world(pocs, plan, env):
    x = Things(pocs, plan, env)
    with pocs.Context(0) as c:
        fresh(x, c)
        c.set_world(x.w100)
        p0 = c.run_gmm_estimation()
        texts = check(c, x, [(n, E_STATE) for n in ("OBSTACLE_COUNTS", "MC_FUSED", "set_plan_tree", "set_shard", "gmm_begin", "xchg_create",
                                                     "probe_device_collide", "bind_moments")] + [("addObstacle", E_ARG), ("bind_moments(null)", OK)])
        assert all("world" in t for t in texts)
        assert c.world_boxes() == 100
        run_again(c, p0)
    for opt in ("OBSTACLE_COUNTS", "MC_FUSED"):                                 # the other order: the option first
        with pocs.Context(0) as c:
            fresh(x, c)
            CALLS[opt](c, x)
            p0 = c.run_gmm_estimation()
            check(c, x, [("set_world(100)", E_STATE), ("set_world(64)", OK)])
            c.set_env(env)
            run_again(c, p0)


def test_open_sequence(pocs, plan, env):
    x = Things(pocs, plan, env)
    with pocs.Context(0) as c:
        fresh(x, c)
        p0 = c.run_gmm_estimation()
        c.set_seed(SEED)
        c.gmm_begin()
        check(c, x, [(n, E_ORDER) for n in ("set_batch", "set_plans", "set_plan_tree", "set_plan_risk_bound", "OBSTACLE_COUNTS", "set_world(100)")])
        run_again(c, p0)                                                        # (the sequence stays open: the suite's shared context does the same)
    with pocs.Context(0) as c:                                                  # sharded: the sequence is asked about before the shard
        fresh(x, c)
        c.set_shard(0, 500)
        p0 = c.run_gmm_estimation()
        c.set_seed(SEED)
        c.gmm_begin()
        check(c, x, [("set_plans", E_ORDER)])
        run_again(c, p0)
