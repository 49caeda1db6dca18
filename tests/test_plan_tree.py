"""A tree of candidate plans (pocs_set_plan_tree): one call evaluates every NODE once, and every node gets bit for bit what
pocs_set_plans computes for the path root -> node alone under common random numbers -- which the oracle restates path by
path.  Merging plans into a tree and walking a path back out of it are checked on the CPU; everything that launches is
marked `gpu`."""
import re
from pathlib import Path

import numpy as np
import pytest

SEED = 0x5EED0001
WEYL = 0x9E3779B97F4A7C15            # effective seed of the r-th run of a context = seed + r * WEYL (mod 2^64)
ROOT = Path(__file__).resolve().parents[1]
NEW = ("pocs_set_plan_tree", "pocs_get_tree_probabilities", "pocs_get_tree_evaluated", "pocs_mc_get_tree_counts",
       "pocs_select_tree_node")


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


def branch_plans(pocs, plan):
    """The bundled 56-waypoint plan with three branches at waypoint 20 and, on each of those, two at waypoint 40, plus a
    22-waypoint plan that leaves the trunk at waypoint 20 for a leaf: node 20 has three inner children and a leaf."""
    out = [branch(pocs, branch(pocs, plan, 20, a), 40, b) for a in (0.0, 0.1, -0.1) for b in (0.0, 0.05)]
    short = prefix(plan, 22)
    short["traj"][21, 1] += 0.07
    short["odom"][20:] = pocs.planio.path_odometry(short["traj"][20:])
    return out + [short]


N_TEST_NODES = 21 + 3 * 20 + 6 * 15 + 1


def depths(parent):
    d = np.zeros(len(parent), dtype=int)
    for n in range(1, len(parent)):
        d[n] = d[parent[n]] + 1
    return d


# ---- CPU -----------------------------------------------------------------------------------------------------------

def test_tree_abi_is_declared_exported_and_wrapped(pocs):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pocs.h").read_text(), flags=re.S)
    assert re.search(r"int\s+pocs_set_plan_tree\s*\(\s*pocs_ctx\s*\*\s*ctx\s*,\s*int\s+nodes\s*,\s*const\s+int\s*\*\s*parent\s*,"
                     r"\s*const\s+double\s*\*\s*poses\s*,\s*const\s+double\s*\*\s*odoms\s*\)", text)
    assert re.search(r"int\s+pocs_get_tree_probabilities\s*\(\s*pocs_ctx\s*\*\s*ctx\s*,\s*double\s*\*\s*out\s*,\s*int\s+cap\s*\)", text)
    assert re.search(r"int\s+pocs_get_tree_evaluated\s*\(\s*pocs_ctx\s*\*\s*ctx\s*,\s*unsigned\s+char\s*\*\s*out\s*,\s*int\s+cap\s*\)", text)
    assert re.search(r"int\s+pocs_mc_get_tree_counts\s*\(\s*pocs_ctx\s*\*\s*ctx\s*,\s*unsigned\s+long\s+long\s*\*\s*out\s*,\s*int\s+cap\s*\)", text)
    assert re.search(r"int\s+pocs_select_tree_node\s*\(\s*pocs_ctx\s*\*\s*ctx\s*,\s*int\s+node\s*\)", text)
    for name in NEW:
        assert name in pocs.SIGNATURES, name
    for meth in ("set_plan_tree", "clear_plan_tree", "tree_probabilities", "tree_evaluated", "tree_counts", "select_tree_node"):
        assert callable(getattr(pocs.Context, meth)), meth
    lib = pocs.load_library()
    for name in NEW:
        assert hasattr(lib, name), "libpocs.so does not export %s" % name


def test_tree_from_plans_merges_prefixes(pocs, plan):
    plans = branch_plans(pocs, plan) + [prefix(plan, 30), prefix(plan, 1), prefix(plan, 56)]
    parent, poses, odoms, leaf = pocs.tree_from_plans(plans)
    T = len(parent)
    assert T == N_TEST_NODES                                   # the three prefixes of the trunk add no node
    assert parent.dtype == np.int32 and poses.shape == (T, 3) and odoms.shape == (T, 3) and len(leaf) == len(plans)
    assert parent[0] == -1 and all(0 <= parent[n] < n for n in range(1, T))
    d = depths(parent)
    assert d.max() == 55 and np.count_nonzero(d == 21) == 4 and np.count_nonzero(d == 41) == 6
    kids = [np.flatnonzero(parent == n) for n in range(T)]
    n20 = int(np.flatnonzero(d == 20)[0])
    assert len(kids[n20]) == 4 and sum(len(kids[k]) == 0 for k in kids[n20]) == 1      # a leaf next to inner children
    for pl, n in zip(plans, leaf):
        back = pocs.tree_path(parent, poses, odoms, int(n))
        assert np.array_equal(back["traj"], pl["traj"]) and np.array_equal(back["odom"], np.asarray(pl["odom"]).reshape(-1, 3))
    assert leaf[7] == 29 and leaf[8] == 0 and leaf[9] == leaf[0] == 55          # prefixes end on the trunk's nodes
    # a single plan is a chain
    parent, poses, odoms, leaf = pocs.tree_from_plans([plan])
    assert list(parent) == list(range(-1, 55)) and np.array_equal(poses, plan["traj"]) and np.array_equal(odoms[1:], plan["odom"])
    assert list(leaf) == [55]


@pytest.mark.parametrize("j", [1, 17, 55])
def test_one_bit_of_one_pose_splits_the_tree_there(pocs, plan, j):
    other = dict(traj=np.asarray(plan["traj"]).copy(), odom=np.asarray(plan["odom"]).copy())
    other["traj"][j, 0] = np.nextafter(other["traj"][j, 0], np.inf)        # one bit of one pose of waypoint j
    parent, poses, odoms, leaf = pocs.tree_from_plans([plan, other])
    assert len(parent) == 56 + (56 - j)                                  # waypoints 0 .. j - 1 are shared: exactly j nodes
    d = depths(parent)
    assert [int(np.count_nonzero(d == w)) for w in range(56)] == [1] * j + [2] * (56 - j)
    # ... and so does one bit of one control
    other = dict(traj=np.asarray(plan["traj"]).copy(), odom=np.asarray(plan["odom"]).copy())
    other["odom"][j - 1, 1] = np.nextafter(other["odom"][j - 1, 1], np.inf)
    assert len(pocs.tree_from_plans([plan, other])[0]) == 56 + (56 - j)
    # 0.0 and -0.0 are different bits
    a, b = prefix(plan, 3), prefix(plan, 3)
    a["traj"][2, 2], b["traj"][2, 2] = 0.0, -0.0
    assert len(pocs.tree_from_plans([a, b])[0]) == 4


def test_malformed_trees_raise(pocs, plan):
    parent, poses, odoms, _ = pocs.tree_from_plans([prefix(plan, 6)])
    chk = pocs.planio.check_tree
    chk(parent, poses, odoms)
    two_roots = parent.copy(); two_roots[3] = -1
    forward = parent.copy(); forward[2] = 4
    itself = parent.copy(); itself[2] = 2
    no_root = parent.copy(); no_root[0] = 0
    for bad in (two_roots, forward, itself, no_root):
        with pytest.raises(ValueError):
            chk(bad, poses, odoms)
        with pytest.raises(ValueError):
            pocs.tree_path(bad, poses, odoms, 5)
    with pytest.raises(ValueError):
        chk(parent, poses[:, :2], odoms)
    with pytest.raises(ValueError):
        chk(parent[:0], poses[:0], odoms[:0])
    n = 4097                                                              # more than 4096 nodes
    with pytest.raises(ValueError):
        chk(np.arange(-1, n - 1), np.zeros((n, 3)), np.zeros((n, 3)))
    chk(np.arange(-1, 4095), np.zeros((4096, 3)), np.zeros((4096, 3)))
    star = [dict(traj=np.array([[0.0, 0.0, 0.0], [1.0, float(i), 0.0]]), odom=np.array([[0.0, 1.0, 0.0]])) for i in range(4096)]
    with pytest.raises(ValueError):
        pocs.tree_from_plans(star)                                        # 4097 nodes
    assert len(pocs.tree_from_plans(star[:4095])[0]) == 4096
    with pytest.raises(ValueError):                                       # two roots
        pocs.tree_from_plans([prefix(plan, 3), dict(traj=np.asarray(plan["traj"])[1:4], odom=np.asarray(plan["odom"])[1:3])])
    with pytest.raises(ValueError):
        pocs.tree_from_plans([])
    with pytest.raises(ValueError):
        pocs.tree_path(parent, poses, odoms, 6)


# ---- GPU -----------------------------------------------------------------------------------------------------------

def gmm_view(c, K):
    """What the getters show of the selected node / plan."""
    W = c.path_length()
    chain = c.host_chain(8) if W > 1 else {}
    return dict(W=W, probs=c.waypoint_probabilities().copy(), moments=np.array([c.moments(w, K) for w in range(W)]),
                states=np.array([c.gmm_state_raw(w, K) for w in range(W)])[..., :14], **chain)


def same_view(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def running(probs):
    prod = 1.0
    for p in probs:
        prod *= (1.0 - p)
    return 1.0 - prod


def fresh(pocs, plan, env, K, N, seed=SEED):
    c = pocs.Context(0)
    c.configure(plan, env, K=K, N=N, seed=seed)
    c.set_option(pocs.OPT_PLAN_SEEDS, 1)
    return c


def check_gmm_tree_against_paths(pocs, plan, env, tree, K, N, calls=1, nodes=None):
    """`calls` consecutive GMM calls on the tree == the same number of consecutive set_plans([path]) calls, node by node."""
    parent, poses, odoms = tree
    T = len(parent)
    nodes = range(T) if nodes is None else nodes
    got = []
    with fresh(pocs, plan, env, K, N) as c:
        c.set_plan_tree(parent, poses, odoms)
        for _ in range(calls):
            p0 = c.run_gmm_estimation()
            finals = c.tree_probabilities().copy()
            assert len(finals) == T and p0 == finals[0]
            assert c.tree_evaluated().tolist() == [1] * T
            views = {}
            for n in nodes:
                c.select_tree_node(n)
                views[n] = gmm_view(c, K)
            with pytest.raises(pocs.PocsError) as e:
                c.gmm_samples(N)                       # a call on a tree stores no samples
            assert e.value.code == pocs.capi.E_STATE
            got.append((finals, views))
    d = depths(parent)
    with fresh(pocs, plan, env, K, N) as ref:
        for n in nodes:
            ref.set_plans([pocs.tree_path(parent, poses, odoms, n)])
            ref.set_seed(SEED)
            for call in range(calls):
                p = ref.run_gmm_estimation()
                finals, views = got[call]
                want = gmm_view(ref, K)
                assert want["W"] == d[n] + 1
                assert finals[n] == p == running(views[n]["probs"]), (n, call)
                assert same_view(views[n], want), (n, call)
            ref.clear_plans()
    return got


def tree_of_branch_plans(pocs, plan):
    parent, poses, odoms, leaf = pocs.tree_from_plans(branch_plans(pocs, plan))
    assert len(parent) == N_TEST_NODES >= 150 and depths(parent).max() == 55
    return (parent, poses, odoms), leaf


@pytest.mark.gpu
def test_gmm_tree_equals_its_paths(pocs, orc, plan, env):
    K, N = 3, 100000
    tree, leaf = tree_of_branch_plans(pocs, plan)
    got = check_gmm_tree_against_paths(pocs, plan, env, tree, K, N, calls=2)
    d = depths(tree[0])
    inner = int(np.flatnonzero(d == 30)[1])
    for call in (0, 1):
        finals, views = got[call]
        assert len(set(finals[leaf].tolist())) > 2, finals[leaf]              # the branches are told apart
        for n in (0, inner, int(leaf[5])):                                    # the root, an inner node, the deepest leaf
            cfg = orc.config(pocs.tree_path(*tree, n), env, K=K)
            want = orc.run_gmm(cfg, seed_of(call), N)
            v = views[n]
            assert finals[n] == want["prob"], (n, call)
            assert np.array_equal(v["probs"], want["probs"]) and np.array_equal(v["moments"], want["moments"]), (n, call)
            assert np.array_equal(v["states"], want["states"][..., :14]), (n, call)
            if v["W"] > 1:
                wc = orc.host_chain(cfg, seed_of(call))
                for k in ("applied", "noisy", "z", "mu", "cov"):
                    assert np.array_equal(v[k], wc[k]), (n, call, k)


def mc_view(c, N, particles):
    out = dict(W=c.path_length(), wp=c.mc_waypoint_counts().copy())
    if particles:
        out["xyz"], out["hits"] = c.particles(N)
    return out


@pytest.mark.gpu
def test_mc_tree_equals_its_paths(pocs, orc, plan, env):
    K, N = 3, 20000
    (parent, poses, odoms), leaf = tree_of_branch_plans(pocs, plan)
    T, d = len(parent), depths(parent)
    deepest = [int(n) for n in np.flatnonzero(d == d.max())]
    got = {}
    with fresh(pocs, plan, env, K, N) as c:
        c.set_option(pocs.OPT_MC_WAYPOINT_COUNTS, 1)
        c.set_plan_risk_bound(0.2)                       # an MC call on a tree ignores the bound, with the option too
        c.set_option(pocs.OPT_MC_RISK_BOUND, 1)
        c.set_plan_tree(parent, poses, odoms)
        for fused in (0, 1):
            c.set_option(pocs.OPT_MC_FUSED, fused)
            c.set_seed(SEED)
            p0 = c.run_simulation()
            counts = c.tree_counts().copy()
            assert len(counts) == T and p0 == counts[0] / N
            assert np.array_equal(c.tree_probabilities(), counts / float(N)) and c.tree_evaluated().tolist() == [1] * T
            views = {}
            for n in range(T):
                c.select_tree_node(n)
                views[n] = mc_view(c, N, n in deepest)
                if n not in deepest and n % 40 == 0:
                    with pytest.raises(pocs.PocsError) as e:
                        c.particles(N)
                    assert e.value.code == pocs.capi.E_STATE
            got[fused] = (counts, views)
    assert np.array_equal(got[0][0], got[1][0])
    assert all(same_view(got[0][1][n], got[1][1][n]) for n in range(T))
    assert len(set(got[0][0][leaf].tolist())) > 2
    inner = int(np.flatnonzero(d == 30)[1])
    with fresh(pocs, plan, env, K, N) as ref:
        ref.set_option(pocs.OPT_MC_WAYPOINT_COUNTS, 1)
        for n in range(T):
            path = pocs.tree_path(parent, poses, odoms, n)
            ref.set_plans([path])
            for fused in ((0, 1) if n in (0, inner, deepest[-1]) else (0,)):
                ref.set_option(pocs.OPT_MC_FUSED, fused)
                ref.set_seed(SEED)
                p = ref.run_simulation()
                want = mc_view(ref, N, n in deepest)
                counts, views = got[fused]
                assert counts[n] == ref.mc_batch_counts()[0] == int(want["wp"].sum()) and p == counts[n] / N, (n, fused)
                assert same_view(views[n], want), (n, fused)
            ref.clear_plans()
            if n in (0, inner, deepest[-1]):
                n_orc, hits, parts = orc.run_mc(orc.config(path, env, K=K), SEED, N, want_particles=True)
                assert got[0][0][n] == n_orc == np.count_nonzero(hits), n
                if n in deepest:
                    assert np.array_equal(got[0][1][n]["hits"], hits) and np.array_equal(got[0][1][n]["xyz"], parts)


@pytest.mark.gpu
def test_wide_levels_and_long_chains(pocs, plan, env):
    # a star: 600 children of the root, a level wider than one launch's 256 runs
    root = np.asarray(plan["traj"])[0]
    kids = np.array([root + np.array([0.05 + 0.0005 * i, 0.4 * np.sin(0.7 * i), 0.0]) for i in range(600)])
    parent = np.array([-1] + [0] * 600, dtype=np.int32)
    poses = np.vstack([root[None, :], kids])
    odoms = np.vstack([np.zeros((1, 3)), [pocs.planio.inverse_odometry(root, k) for k in kids]])
    star = (parent, poses, odoms)
    check_gmm_tree_against_paths(pocs, plan, env, star, 3, 20000)
    # a chain: one node per level, depth 120, K = 2
    long = pocs.resample_plan(plan, 121)
    parent, poses, odoms, leaf = pocs.tree_from_plans([long])
    assert list(leaf) == [120] and depths(parent).max() == 120
    check_gmm_tree_against_paths(pocs, plan, env, (parent, poses, odoms), 2, 20000)
    # the same two trees on the MC path
    for tree in (star, (parent, poses, odoms)):
        T, N = len(tree[0]), 20000
        with fresh(pocs, plan, env, 2, N) as c:
            c.set_plan_tree(*tree)
            c.run_simulation()
            counts = c.tree_counts().copy()
            wps = []
            for n in range(T):
                c.select_tree_node(n)
                wps.append(c.mc_waypoint_counts().copy())
        with fresh(pocs, plan, env, 2, N) as ref:
            ref.set_option(pocs.OPT_MC_WAYPOINT_COUNTS, 1)
            for n in range(T):
                ref.set_plans([pocs.tree_path(*tree, n)])
                ref.set_seed(SEED)
                ref.run_simulation()
                assert counts[n] == ref.mc_batch_counts()[0], n
                assert np.array_equal(wps[n], ref.mc_waypoint_counts()), n
                ref.clear_plans()


@pytest.mark.gpu
def test_risk_bound_cuts_subtrees(pocs, orc, plan, env):
    """Oracle, K = 3, N = 10^5, this seed: the leaves of the three branches at waypoint 20 end at 0.298, 0.532 and 0.978 and
    the short plan's leaf at 0.134, so the median of the leaves' probabilities stops the second and third branch (both before
    waypoint 40) and leaves the trunk's branch and the short plan alone."""
    K, N = 3, 100000
    (parent, poses, odoms), leaf = tree_of_branch_plans(pocs, plan)
    T = len(parent)
    with fresh(pocs, plan, env, K, N) as c:
        c.set_plan_tree(parent, poses, odoms)
        c.run_gmm_estimation()
        free = c.tree_probabilities().copy()
        views = {}
        for n in range(T):
            c.select_tree_node(n)
            views[n] = gmm_view(c, K)
        for n, p in zip(leaf, (0.297627, 0.297627, 0.531755, 0.531755, 0.978041, 0.978034, 0.134131)):
            assert abs(free[n] - p) < 5e-7, (n, free[n], p)            # the docstring's figures (the oracle's, to six places)
        bound = float(np.median(free[leaf]))
        c.set_plan_risk_bound(bound)
        c.set_seed(SEED)
        p0 = c.run_gmm_estimation()
        probs, ev = c.tree_probabilities().copy(), c.tree_evaluated().copy()
        assert p0 == probs[0] and len(ev) == T
        # the rule, restated on the unbounded call: a node is evaluated unless an ancestor has reached the bound
        want_ev, anc = np.ones(T, dtype=np.uint8), np.full(T, -1)       # anc: the stopped ancestor of an unevaluated node
        for n in range(1, T):
            p = parent[n]
            if not want_ev[p]:
                want_ev[n], anc[n] = 0, anc[p]
            elif free[p] >= bound:
                want_ev[n], anc[n] = 0, p
        assert np.array_equal(ev, want_ev)
        stopped_leaves = [int(n) for n in leaf if not ev[n]]
        live_leaves = [int(n) for n in leaf if ev[n]]
        assert stopped_leaves and live_leaves, (stopped_leaves, live_leaves)       # some subtrees stop, some do not
        for n in range(T):
            if ev[n]:
                assert probs[n] == free[n], n
                c.select_tree_node(n)
                assert same_view(gmm_view(c, K), views[n]), n
            else:
                assert probs[n] == free[anc[n]] >= bound, n
                c.select_tree_node(n)
                assert c.path_length() == depths(parent)[n] + 1
                assert np.array_equal(c.waypoint_probabilities(), views[anc[n]]["probs"]), n     # the evaluated part of its path
                with pytest.raises(pocs.PocsError) as e:
                    c.gmm_state(c.path_length() - 1, K)
                assert e.value.code == pocs.capi.E_ARG
        # the bound off again: the unbounded call
        c.set_plan_risk_bound(1.0)
        c.set_seed(SEED)
        c.run_gmm_estimation()
        assert np.array_equal(c.tree_probabilities(), free) and c.tree_evaluated().tolist() == [1] * T


@pytest.mark.gpu
def test_nothing_else_moved(pocs, plan, env):
    K, N = 3, 30000
    (parent, poses, odoms), leaf = tree_of_branch_plans(pocs, plan)
    plans = [prefix(plan, 20), plan, prefix(plan, 7)]

    def single_and_plans(c):
        out = []
        c.set_seed(SEED)
        out.append(np.float64(c.run_gmm_estimation()))
        out.append(c.waypoint_probabilities().copy())
        out.append(np.array([c.gmm_state_raw(w, K) for w in (0, 30, 55)]))
        out.append(np.float64(c.run_simulation()))
        c.set_plans(plans)
        c.set_seed(SEED)
        c.run_gmm_estimation()
        out.append(c.batch_probabilities().copy())
        for p in range(len(plans)):
            c.select_batch_run(p)
            out.append(c.waypoint_probabilities().copy())
        c.run_simulation()
        out.append(np.array(c.mc_batch_counts()))
        c.clear_plans()
        return out

    with pocs.Context(0) as c:
        c.configure(plan, env, K=K, N=N, seed=SEED)
        c.set_plan_tree(parent, poses, odoms)
        assert c.path_length() == 1
        c.run_gmm_estimation()
        c.run_simulation()
        for call in (lambda: c.set_plans(plans), lambda: c.set_batch(4), lambda: c.set_plan(plan), lambda: c.select_batch_run(0)):
            with pytest.raises(pocs.PocsError) as e:
                call()
            assert e.value.code == pocs.capi.E_ORDER
        for call in (lambda: c.set_shard(0, N // 2), c.gmm_begin, lambda: c.xchg_create(2, 0)):
            with pytest.raises(pocs.PocsError) as e:
                call()
            assert e.value.code == pocs.capi.E_STATE
        with pytest.raises(pocs.PocsError) as e:
            c.select_tree_node(len(parent))
        assert e.value.code == pocs.capi.E_ARG
        c.run_gmm_estimation()                           # the refused calls left the tree as it was
        assert len(c.tree_probabilities()) == len(parent)
        c.clear_plan_tree()
        assert c.path_length() == 56
        with pytest.raises(pocs.PocsError) as e:
            c.tree_probabilities()
        assert e.value.code == pocs.capi.E_STATE
        after = single_and_plans(c)
        c.set_plans(plans)                               # ... and the reverse
        with pytest.raises(pocs.PocsError) as e:
            c.set_plan_tree(parent, poses, odoms)
        assert e.value.code == pocs.capi.E_ORDER
        c.clear_plans()
        bad = parent.copy()
        bad[5] = 7
        rc = c.lib.pocs_set_plan_tree(c.h, len(bad), bad.ctypes.data_as(pocs.capi.C.POINTER(pocs.capi.C.c_int)),
                                      poses.T.copy().ctypes.data_as(pocs.capi._dp), odoms.T.copy().ctypes.data_as(pocs.capi._dp))
        assert rc == pocs.capi.E_ARG
        rc = c.lib.pocs_set_plan_tree(c.h, 4097, None, None, None)
        assert rc == pocs.capi.E_ARG
    with pocs.Context(0) as c:
        c.configure(plan, env, K=K, N=N, seed=SEED)
        want = single_and_plans(c)
    assert len(after) == len(want) and all(np.array_equal(a, b) for a, b in zip(after, want))
