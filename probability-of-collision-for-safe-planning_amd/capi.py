"""ctypes binding of the C ABI declared in include/pocs.h (libpocs.so).

Nothing here computes: every call goes into the HIP library.  If libpocs.so is missing it is
built with hipcc (build.py); if that is impossible, or no GPU is usable, the error is raised --
there is no CPU fallback.
"""
import ctypes as C
from pathlib import Path

import numpy as np

from . import build as _build

POCS_OK = 0
E_ARG, E_ORDER, E_STATE, E_DEVICE, E_UNKNOWN_COMMAND, E_BUFFER = -1, -2, -3, -4, -5, -6
OPT_STORE_SAMPLES, OPT_MC_FUSED, OPT_USE_GRAPH, OPT_PROFILE, OPT_RUN_AHEAD, OPT_PERSISTENT, OPT_LONE_CALL = 1, 2, 3, 4, 5, 6, 7
OPT_SUB_BATCHES, OPT_MC_NONTEMPORAL, OPT_PLAN_SEEDS, OPT_MC_WAYPOINT_COUNTS, OPT_MC_RISK_BOUND = 8, 9, 10, 11, 12
OPT_OBSTACLE_COUNTS = 13
MAX_OBSTACLES = 64                 # POCS_MAX_OBSTACLES: the widest table pocs_get_obstacle_counts writes
NMOM = 11
MAX_PLANS = 256
MAX_TREE_NODES = 4096
MAX_WORLD_STEPS = 4096
MAX_WORLD_BOXES = 4096             # POCS_MAX_WORLD_BOXES: the largest table pocs_set_world takes
MAX_CLEARANCE_LEVELS = 4           # POCS_MAX_CLEARANCE_LEVELS: the most distances pocs_set_clearance_levels takes
MAX_REGIONS = 4                    # POCS_MAX_REGIONS: the most boxes pocs_set_regions takes
MAX_SEGMENT_CHECKS = 8             # POCS_MAX_SEGMENT_CHECKS: the most checks per segment pocs_set_segment_checks takes
REGION_TOUCH, REGION_POINT = 0, 1  # POCS_REGION_*: the robot's footprint touches the box / the pose's reference point lies in it
MAX_FOOTPRINT_PARTS = 4            # POCS_MAX_FOOTPRINT_PARTS: the most parts pocs_set_footprint_parts takes

_dp = C.POINTER(C.c_double)
_vp = C.c_void_p

# name -> (restype, argtypes); the authoritative list is include/pocs.h (tests check both agree)
SIGNATURES = {
    "pocs_create": (C.c_int, [C.POINTER(_vp), C.c_int]),
    "pocs_destroy": (None, [_vp]),
    "pocs_last_error": (C.c_char_p, [_vp]),
    "pocs_version": (C.c_char_p, []),
    "pocs_set_footprint": (C.c_int, [_vp, C.c_double, C.c_double, C.c_double, C.c_double]),
    "pocs_set_obstacles": (C.c_int, [_vp, _dp, C.c_int]),
    "pocs_set_obstacle_schedule": (C.c_int, [_vp, _dp, C.c_int, C.c_int]),
    "pocs_get_world_steps": (C.c_int, [_vp]),
    "pocs_set_world": (C.c_int, [_vp, _dp, C.c_int]),
    "pocs_get_world_boxes": (C.c_int, [_vp]),
    "pocs_get_world_reach": (C.c_int, [_vp, C.POINTER(C.c_int), C.c_int]),
    "pocs_set_alphas": (C.c_int, [_vp, _dp, C.c_int]),
    "pocs_set_q": (C.c_int, [_vp, C.c_double]),
    "pocs_set_num_landmarks": (C.c_int, [_vp, C.c_int]),
    "pocs_set_landmarks": (C.c_int, [_vp, _dp, C.c_int]),
    "pocs_set_num_particles": (C.c_int, [_vp, C.c_longlong]),
    "pocs_set_initial_covariance": (C.c_int, [_vp, _dp]),
    "pocs_set_path_length": (C.c_int, [_vp, C.c_int]),
    "pocs_set_trajectory": (C.c_int, [_vp, _dp, C.c_int]),
    "pocs_set_odometry": (C.c_int, [_vp, _dp, C.c_int]),
    "pocs_set_num_gaussians": (C.c_int, [_vp, C.c_int]),
    "pocs_set_num_gmm_samples": (C.c_int, [_vp, C.c_longlong]),
    "pocs_set_seed": (C.c_int, [_vp, C.c_uint64]),
    "pocs_run_simulation": (C.c_int, [_vp, _dp]),
    "pocs_run_gmm_estimation": (C.c_int, [_vp, _dp]),
    "pocs_send_command": (C.c_int, [_vp, C.c_char_p, C.c_char_p, C.c_size_t]),
    "pocs_set_option": (C.c_int, [_vp, C.c_int, C.c_longlong]),
    "pocs_set_batch": (C.c_int, [_vp, C.c_int]),
    "pocs_get_batch_probabilities": (C.c_int, [_vp, _dp, C.c_int]),
    "pocs_select_batch_run": (C.c_int, [_vp, C.c_int]),
    "pocs_set_plans": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int), _dp, _dp]),
    "pocs_set_plan_risk_bound": (C.c_int, [_vp, C.c_double]),
    "pocs_get_plan_evaluated": (C.c_int, [_vp, C.POINTER(C.c_int), C.c_int]),
    "pocs_set_plan_tree": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int), _dp, _dp]),
    "pocs_get_tree_probabilities": (C.c_int, [_vp, _dp, C.c_int]),
    "pocs_get_tree_evaluated": (C.c_int, [_vp, C.POINTER(C.c_ubyte), C.c_int]),
    "pocs_mc_get_tree_counts": (C.c_int, [_vp, C.POINTER(C.c_ulonglong), C.c_int]),
    "pocs_select_tree_node": (C.c_int, [_vp, C.c_int]),
    "pocs_set_shard": (C.c_int, [_vp, C.c_longlong, C.c_longlong]),
    "pocs_set_stream": (C.c_int, [_vp, _vp]),
    "pocs_gmm_begin": (C.c_int, [_vp]),
    "pocs_gmm_step_local": (C.c_int, [_vp, C.c_int]),
    "pocs_gmm_advance_local": (C.c_int, [_vp, C.c_int]),
    "pocs_gmm_sample_local": (C.c_int, [_vp, C.c_int]),
    "pocs_gmm_moments_ptr": (_vp, [_vp, C.c_int]),
    "pocs_gmm_moments_len": (C.c_int, [_vp]),
    "pocs_gmm_bind_moments": (C.c_int, [_vp, _vp, C.c_longlong]),
    "pocs_gmm_end": (C.c_int, [_vp, _dp]),
    "pocs_mc_run_local": (C.c_int, [_vp, C.POINTER(C.c_ulonglong)]),
    "pocs_mc_get_batch_counts": (C.c_int, [_vp, C.POINTER(C.c_ulonglong), C.c_int]),
    "pocs_mc_get_waypoint_counts": (C.c_int, [_vp, C.POINTER(C.c_ulonglong), C.c_int]),
    "pocs_get_obstacle_counts": (C.c_int, [_vp, C.POINTER(C.c_ulonglong), C.c_int, C.POINTER(C.c_int)]),
    "pocs_set_clearance_levels": (C.c_int, [_vp, _dp, C.c_int]),
    "pocs_get_clearance_levels": (C.c_int, [_vp, _dp, C.c_int]),
    "pocs_get_clearance_counts": (C.c_int, [_vp, C.POINTER(C.c_ulonglong), C.c_int, C.POINTER(C.c_int)]),
    "pocs_get_batch_clearance_probabilities": (C.c_int, [_vp, C.c_int, _dp, C.c_int]),
    "pocs_probe_device_clearance": (C.c_int, [_vp, _dp, _dp, C.c_int, _dp, C.c_int, C.c_int, _dp, C.POINTER(C.c_int)]),
    "pocs_set_footprint_parts": (C.c_int, [_vp, _dp, C.c_int]),
    "pocs_get_footprint_parts": (C.c_int, [_vp, _dp, C.c_int]),
    "pocs_set_regions": (C.c_int, [_vp, _dp, C.POINTER(C.c_int), C.c_int]),
    "pocs_get_regions": (C.c_int, [_vp, _dp, C.POINTER(C.c_int), C.c_int]),
    "pocs_get_region_counts": (C.c_int, [_vp, C.POINTER(C.c_ulonglong), C.c_int, C.POINTER(C.c_int)]),
    "pocs_get_batch_region_probabilities": (C.c_int, [_vp, C.c_int, C.c_int, _dp, C.c_int]),
    "pocs_probe_device_regions": (C.c_int, [_vp, _dp, _dp, C.POINTER(C.c_int), C.c_int, C.c_int, _dp, C.POINTER(C.c_int)]),
    "pocs_set_discs": (C.c_int, [_vp, _dp, C.c_int, C.c_int]),
    "pocs_get_discs": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "pocs_probe_device_discs": (C.c_int, [_vp, _dp, _dp, C.c_int, _dp, C.c_int, C.c_int, _dp, C.POINTER(C.c_int)]),
    "pocs_set_footprint_disc": (C.c_int, [_vp, C.c_double]),
    "pocs_get_footprint_disc": (C.c_int, [_vp, _dp]),
    "pocs_probe_device_footprint_disc": (C.c_int, [_vp, C.c_double, _dp, C.c_int, _dp, C.c_int, _dp, C.c_uint64, C.c_uint32, C.c_ulonglong, C.c_int, _dp,
                                                   C.POINTER(C.c_int)]),
    "pocs_set_disc_covariances": (C.c_int, [_vp, _dp, C.c_int, C.c_int, C.c_int]),
    "pocs_get_disc_covariances": (C.c_int, [_vp, _dp, C.c_int, C.POINTER(C.c_int)]),
    "pocs_probe_device_disc_noise": (C.c_int, [_vp, _dp, _dp, _dp, C.c_int, C.c_uint64, C.c_uint32, C.c_ulonglong, C.c_int, _dp, _dp, C.POINTER(C.c_uint)]),
    "pocs_set_disc_hypotheses": (C.c_int, [_vp, C.POINTER(C.c_int), _dp, C.c_int]),
    "pocs_get_disc_hypotheses": (C.c_int, [_vp, C.POINTER(C.c_int), _dp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.c_int]),
    "pocs_probe_device_disc_hypotheses": (C.c_int, [_vp, _dp, _dp, _dp, C.POINTER(C.c_int), _dp, C.c_int, C.c_uint64, C.c_uint32, C.c_ulonglong, C.c_int, _dp,
                                                    C.POINTER(C.c_uint), C.POINTER(C.c_uint)]),
    "pocs_set_segment_checks": (C.c_int, [_vp, C.c_int]),
    "pocs_get_segment_checks": (C.c_int, [_vp]),
    "pocs_get_segment_counts": (C.c_int, [_vp, C.POINTER(C.c_ulonglong), C.c_int]),
    "pocs_probe_device_segment": (C.c_int, [_vp, _dp, _dp, C.c_int, _dp, C.c_int, C.c_int, C.c_int, _dp, C.POINTER(C.c_int)]),
    "pocs_probe_device_footprint_parts": (C.c_int, [_vp, _dp, C.c_int, _dp, C.c_int, C.c_int, _dp, C.POINTER(C.c_int)]),
    "pocs_xchg_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_void_p]),
    "pocs_xchg_connect": (C.c_int, [_vp, C.c_void_p, C.c_int]),
    "pocs_gmm_exchange_local": (C.c_int, [_vp, C.c_int]),
    "pocs_gmm_sample_exchange_local": (C.c_int, [_vp, C.c_int]),
    "pocs_get_path_length": (C.c_int, [_vp]),
    "pocs_get_waypoint_probabilities": (C.c_int, [_vp, _dp, C.c_int]),
    "pocs_get_moments": (C.c_int, [_vp, C.c_int, _dp, C.c_int]),
    "pocs_get_gmm_state": (C.c_int, [_vp, C.c_int, _dp, _dp, _dp, _dp]),
    "pocs_get_host_chain": (C.c_int, [_vp, _dp, _dp, _dp, _dp, _dp]),
    "pocs_copy_gmm_samples": (C.c_longlong, [_vp, _dp, C.POINTER(C.c_int16), C.c_longlong]),
    "pocs_copy_particles": (C.c_longlong, [_vp, _dp, C.POINTER(C.c_uint32), C.c_longlong]),
    "pocs_measure_copy_bandwidth": (C.c_int, [_vp, C.c_longlong, _dp]),
    "pocs_measure_fill_bandwidth": (C.c_int, [_vp, C.c_longlong, _dp]),
    "pocs_get_kernel_time": (C.c_int, [_vp, _dp, C.POINTER(C.c_longlong)]),
    "pocs_get_sequence_time": (C.c_int, [_vp, _dp, C.POINTER(C.c_int)]),
    "pocs_get_exchange_wait": (C.c_int, [_vp, _dp]),
    "pocs_get_graph_captures": (C.c_int, [_vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "pocs_probe_device_math": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _dp, _dp, _dp, _dp, _dp, _dp]),
    "pocs_probe_device_radius_roots": (C.c_int, [_vp, C.c_uint32, C.c_ulonglong, C.POINTER(C.c_ulonglong), C.POINTER(C.c_uint32)]),
    "pocs_probe_device_collide": (C.c_int, [_vp, C.c_int, _dp, C.c_int, _dp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                            C.POINTER(C.c_int), _dp]),
    "pocs_probe_device_counts": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int), _dp, _dp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                           C.POINTER(C.c_longlong), _dp]),
}

_lib = None


def library_path():
    return _build.LIB


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  A PyTorch-ROCm wheel carries its own libamdhip64.so (soname
    libamdhip64.so.7, the same as /opt/rocm's) and asks for it by FILE name: imported after libpocs.so
    has pulled in /opt/rocm/lib/libamdhip64.so.7 it loads a second runtime, whose hipInit then finds
    "no ROCm-capable device".  The other order is fine (libpocs.so asks by soname and binds to the copy
    already loaded), so where such a wheel is installed its runtime is mapped first -- without importing
    torch.  No torch: nothing happens, the system runtime serves libpocs.so."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    for loc in (spec.submodule_search_locations or []) if spec else []:
        rt = Path(loc) / "lib" / "libamdhip64.so"
        if rt.exists():
            try:
                C.CDLL(str(rt), mode=C.RTLD_GLOBAL)
            except OSError:
                pass
            return


def load_library(build=True):
    """dlopen libpocs.so (building it first if needed) and declare every prototype."""
    global _lib
    if _lib is not None:
        return _lib
    import os
    path = os.environ.get("POCS_LIB")          # tuning only: an alternative build of the same library
    if not path:
        if build:
            _build.build_library()
        path = str(_build.LIB)
    if not Path(path).exists():
        raise RuntimeError("libpocs.so is missing and was not built; the HIP path is the only path")
    _share_hip_runtime_with_torch()
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        if os.environ.get("POCS_LIB") and not hasattr(lib, name):
            continue                 # tuning only: an A/B build from an older commit may predate an entry point
        fn = getattr(lib, name)      # AttributeError here = header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class PocsError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("pocs error %d: %s" % (code, text))
        self.code = code


def _arr(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _rows(a, width):
    """Records for a probe (None: none of them) -> a contiguous float64 array of rows `width` wide."""
    return np.ascontiguousarray(_arr(a if a is not None else []).reshape(-1, width))


def _dp_or_null(a):
    """The array's data as a double*, NULL for an empty array."""
    return a.ctypes.data_as(_dp) if a.size else None


def pack_plans(plans):
    """Candidate plans ({"traj": W x 3, "odom": (W-1) x 3} each, as set_plan takes one) -> (W, trajs, odoms) as
    pocs_set_plans takes them: W int32[P]; trajs = plan p's trajectory by component (x_0..x_{W-1}, y.., theta..),
    the plans one after the other; odoms = its odometry by component (r1.., tr.., r2..), concatenated the same way."""
    plans = list(plans)
    if not 1 <= len(plans) <= MAX_PLANS:
        raise ValueError("between 1 and %d plans, got %d" % (MAX_PLANS, len(plans)))
    Ws, trajs, odoms = [], [], []
    for i, pl in enumerate(plans):
        t = np.asarray(pl["traj"], dtype=np.float64)
        o = np.asarray(pl["odom"], dtype=np.float64)
        if t.ndim != 2 or t.shape[1] != 3 or t.shape[0] < 1:
            raise ValueError("plan %d: trajectory of shape %s, W x 3 with W >= 1 expected" % (i, t.shape))
        W = t.shape[0]
        if o.size == 0 and W == 1:
            o = o.reshape(0, 3)
        if o.ndim != 2 or o.shape != (W - 1, 3):
            raise ValueError("plan %d: odometry of shape %s, (%d, 3) expected" % (i, o.shape, W - 1))
        Ws.append(W)
        trajs.append(t.T.ravel())
        odoms.append(o.T.ravel())
    return (np.array(Ws, dtype=np.int32), _arr(np.concatenate(trajs)), _arr(np.concatenate(odoms)))


class Context:
    """One estimator context on one GPU (the counterpart of one MCModule + its MCSimulator)."""

    def __init__(self, device=0):
        self.lib = load_library()
        h = _vp()
        rc = self.lib.pocs_create(C.byref(h), device)
        self.h = h
        if rc != POCS_OK:
            msg = self.lib.pocs_last_error(h).decode() if h else "allocation failed"
            if h:
                self.lib.pocs_destroy(h)
            self.h = None
            raise PocsError(rc, msg)

    def close(self):
        if getattr(self, "h", None):
            self.lib.pocs_destroy(self.h)
            self.h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _chk(self, rc):
        if rc < 0:
            raise PocsError(rc, self.lib.pocs_last_error(self.h).decode())
        return rc

    # ---- text channel (MCModule.SendCommand) ------------------------------------------
    def send_command(self, line, cap=1 << 16):
        buf = C.create_string_buffer(cap)
        self._chk(self.lib.pocs_send_command(self.h, line.encode(), buf, cap))
        return buf.value.decode()

    SendCommand = send_command

    # ---- typed setters ----------------------------------------------------------------
    def set_env(self, env):
        if env.get("footprint_radius") is not None:      # a round footprint (set_footprint_disc) in place of any box
            self.set_footprint_disc(env["footprint_radius"])
        elif "footprint_parts" in env:      # a compound footprint (set_footprint_parts) in place of the single box
            self.set_footprint_parts(env["footprint_parts"])
        else:
            fp = env["footprint"]
            self._chk(self.lib.pocs_set_footprint(self.h, fp[0], fp[1], fp[2], fp[3]))
        if env.get("boxes") is None:        # footprint only: the world itself is left as it is
            return
        b = _arr(env["boxes"]).reshape(-1, 5)
        self._chk(self.lib.pocs_set_obstacles(self.h, b.ctypes.data_as(_dp), b.shape[0]))

    def set_obstacle_schedule(self, boxes):
        """Moving obstacles: boxes of shape (S, M, 5), world s = boxes[s] the collision world at waypoint s; waypoints >= S
        see the last world (include/pocs.h).  planio.moving_boxes builds one from velocities."""
        b = _arr(boxes)
        if b.ndim != 3 or b.shape[2] != 5:
            raise ValueError("obstacle schedule of shape %s, (S, M, 5) expected" % (b.shape,))
        self._chk(self.lib.pocs_set_obstacle_schedule(self.h, b.ctypes.data_as(_dp) if b.size else None, b.shape[1], b.shape[0]))

    def world_steps(self):
        """S of the obstacle schedule in force (under discs: the larger of the boxes' and the discs' steps); 1 for a static world; 0
        for a context without a collision world."""
        return self.lib.pocs_get_world_steps(self.h)

    def set_discs(self, discs):
        """Round obstacles beside the boxes: discs of shape (D, 3) = {cx, cy, r} for a static table, or (S, D, 3) for a schedule of
        their own -- table min(w, S - 1) is in force at waypoint w, whatever the boxes' schedule (include/pocs.h).  An empty array or
        None clears.  planio.moving_discs builds a schedule from per-waypoint centres."""
        if discs is None:
            self._chk(self.lib.pocs_set_discs(self.h, None, 0, 0))
            return
        d = _arr(discs)
        if d.size == 0:
            self._chk(self.lib.pocs_set_discs(self.h, None, 0, 0))
            return
        if d.ndim == 2:
            d = d.reshape((1,) + d.shape)
        if d.ndim != 3 or d.shape[2] != 3:
            raise ValueError("discs of shape %s, (D, 3) or (S, D, 3) expected" % (d.shape,))
        d = np.ascontiguousarray(d)
        self._chk(self.lib.pocs_set_discs(self.h, d.ctypes.data_as(_dp), d.shape[1], d.shape[0]))

    def discs(self):
        """(D, S) of the discs in force; (0, 0) without discs."""
        D, S = C.c_int(0), C.c_int(0)
        self._chk(self.lib.pocs_get_discs(self.h, C.byref(D), C.byref(S)))
        return D.value, S.value

    def set_disc_covariances(self, cov, persistent=False):
        """Uncertain discs: a position covariance {sxx, sxy, syy} (m^2) per disc, of shape (D, 3) for a static table or (S, D, 3) for a
        schedule; D and S are those of the discs in force (set_discs).  A row of zeros is a certain disc; None, an empty array or all
        zeros clears.  `persistent` (the MC path): True, a particle's world keeps its deviation from waypoint to waypoint, so a
        covariance that grows is a prediction that fans out; False, the deviations are independent per waypoint -- as the GMM path
        always treats them (include/pocs.h).  planio.prediction_covariances builds a constant-velocity predictor's fan."""
        if cov is None or _arr(cov).size == 0:
            self._chk(self.lib.pocs_set_disc_covariances(self.h, None, 0, 0, 0))
            return
        v = _arr(cov)
        if v.ndim == 2:
            v = v.reshape((1,) + v.shape)
        if v.ndim != 3 or v.shape[2] != 3:
            raise ValueError("covariances of shape %s, (D, 3) or (S, D, 3) expected" % (v.shape,))
        v = np.ascontiguousarray(v)
        self._chk(self.lib.pocs_set_disc_covariances(self.h, v.ctypes.data_as(_dp), v.shape[1], v.shape[0], 1 if persistent else 0))

    def disc_covariances(self):
        """(covariances of shape (S, D, 3), persistent) as in force; (None, False) when none are set."""
        D, S = self.discs()
        out = np.zeros(max(S * D * 3, 1))
        per = C.c_int(0)
        n = self.lib.pocs_get_disc_covariances(self.h, out.ctypes.data_as(_dp), S * D * 3, C.byref(per))
        if n < 0:
            self._chk(n)
        if n == 0:
            return None, False
        return out[:n].reshape(S, D, 3), bool(per.value)

    def set_disc_hypotheses(self, group, weight=None):
        """Prediction hypotheses: per disc in force (set_discs) a group and a weight.  group[d] = -1: disc d is always there;
        group[d] = g in [0, D): disc d is one alternative of group g, existing for a pose with probability floor(weight[d] 2^32) / 2^32,
        and the alternatives of a group exclude each other (include/pocs.h).  None, an empty table or all groups -1 clears.
        planio.prediction_modes builds discs, groups and weights from a predictor's weighted tracks."""
        if group is None or np.asarray(group).size == 0:
            self._chk(self.lib.pocs_set_disc_hypotheses(self.h, None, None, 0))
            return
        g = np.ascontiguousarray(group, dtype=np.int32).ravel()
        w = np.ones(g.size) if weight is None else _arr(weight).ravel()
        if w.size != g.size:
            raise ValueError("%d groups and %d weights" % (g.size, w.size))
        self._chk(self.lib.pocs_set_disc_hypotheses(self.h, g.ctypes.data_as(C.POINTER(C.c_int)), w.ctypes.data_as(_dp), g.size))

    def disc_hypotheses(self):
        """(group int32[D], weight float64[D], lo uint64[D], hi uint64[D]) as in force -- disc d exists for a pose iff lo[d] <= u < hi[d]
        for the pose's 32-bit existence word u --; None when none are set."""
        D = max(self.discs()[0], 1)
        g, w = np.zeros(D, dtype=np.int32), np.zeros(D)
        lo, hi = np.zeros(D, dtype=np.uint64), np.zeros(D, dtype=np.uint64)
        n = self.lib.pocs_get_disc_hypotheses(self.h, g.ctypes.data_as(C.POINTER(C.c_int)), w.ctypes.data_as(_dp), lo.ctypes.data_as(C.POINTER(C.c_ulonglong)),
                                              hi.ctypes.data_as(C.POINTER(C.c_ulonglong)), D)
        if n < 0:
            self._chk(n)
        if n == 0:
            return None
        return g[:n], w[:n], lo[:n], hi[:n]

    def probe_device_disc_hypotheses(self, footprint, discs, cov, group, weight, seed, waypoint_word, first, poses):
        """Test hook: prediction hypotheses on the device for the caller's own footprint (dx, dy, hx, hy), discs (D x 3, D <= 32),
        covariances (D x 3, or None) and hypotheses (group, weight: D each).  Pose i of `poses` (n x 3, n even) has index first + i
        (first even).  Returns (exists uint32[n], flags uint32[n]): bit d = disc d exists for pose i, bit d = pose i touches disc d;
        exists 0 with flags all ones = the kernels' two forms disagree (never)."""
        fp = _arr(footprint).ravel()
        d, xyt = _rows(discs, 3), _rows(poses, 3)
        v = None if cov is None else _rows(cov, 3)
        g = np.ascontiguousarray(group, dtype=np.int32).ravel()
        w = _arr(weight).ravel()
        assert fp.size == 4 and (v is None or v.shape == d.shape) and g.size == w.size == d.shape[0]
        exists = np.full(xyt.shape[0], 0xFFFFFFFF, dtype=np.uint32)
        flags = np.full(xyt.shape[0], 0xFFFFFFFF, dtype=np.uint32)
        self._chk(self.lib.pocs_probe_device_disc_hypotheses(self.h, fp.ctypes.data_as(_dp), d.ctypes.data_as(_dp), None if v is None else v.ctypes.data_as(_dp),
                                                             g.ctypes.data_as(C.POINTER(C.c_int)), w.ctypes.data_as(_dp), d.shape[0], C.c_uint64(int(seed)),
                                                             C.c_uint32(int(waypoint_word)), C.c_ulonglong(int(first)), xyt.shape[0], xyt.ctypes.data_as(_dp),
                                                             exists.ctypes.data_as(C.POINTER(C.c_uint)), flags.ctypes.data_as(C.POINTER(C.c_uint))))
        return exists, flags

    def probe_device_disc_noise(self, footprint, discs, cov, seed, waypoint_word, first, poses):
        """Test hook: uncertain discs on the device for the caller's own footprint (dx, dy, hx, hy), discs (D x 3, D <= 16) and
        covariances (D x 3).  Pose i of `poses` (n x 3, n even) has index first + i (first even).  Returns (centres float64[n, D, 2],
        flags uint32[n]): the displaced centres, bit d = pose i touches displaced disc d, bit 31 = the kernels' two forms disagree
        (never)."""
        fp = _arr(footprint).ravel()
        d, v, xyt = _rows(discs, 3), _rows(cov, 3), _rows(poses, 3)
        assert fp.size == 4 and v.shape == d.shape
        centres = np.full((xyt.shape[0], d.shape[0], 2), np.nan)
        flags = np.full(xyt.shape[0], 0xFFFFFFFF, dtype=np.uint32)
        self._chk(self.lib.pocs_probe_device_disc_noise(self.h, fp.ctypes.data_as(_dp), d.ctypes.data_as(_dp), v.ctypes.data_as(_dp), d.shape[0],
                                                        C.c_uint64(int(seed)), C.c_uint32(int(waypoint_word)), C.c_ulonglong(int(first)), xyt.shape[0],
                                                        xyt.ctypes.data_as(_dp), centres.ctypes.data_as(_dp), flags.ctypes.data_as(C.POINTER(C.c_uint))))
        return centres, flags

    def set_footprint_disc(self, radius):
        """A round footprint: the disc of radius `radius` (finite, >= 0; 0 is a point robot) centred on the pose's reference point,
        in place of the box or the compound footprint in force.  The heading is never read by the collision test; set_env with
        "footprint", set_footprint_parts and the text channel's setFootprint return to boxes (include/pocs.h)."""
        self._chk(self.lib.pocs_set_footprint_disc(self.h, float(radius)))

    def footprint_disc(self):
        """The radius of the round footprint in force, or None under a box footprint."""
        r = C.c_double(0.0)
        got = self._chk(self.lib.pocs_get_footprint_disc(self.h, C.byref(r)))
        return r.value if got == 1 else None

    def probe_device_footprint_disc(self, radius, boxes, discs, poses, cov=None, seed=0, waypoint_word=0, first=0):
        """Test hook: per pose (n x 3; the heading is not read) the kinds of obstacle a ROUND footprint of the caller's own radius
        touches on the device, for the caller's own boxes (M x 5), discs (D x 3) and -- where given -- covariances (D x 3): pose i has
        index first + i (first even).  int32[n]: bit 0 = touches some box, bit 1 = touches some disc (displaced where cov says so),
        bit 8 = the kernels' two forms disagree (never)."""
        b, d, xyt = _rows(boxes, 5), _rows(discs, 3), _rows(poses, 3)
        v = None if cov is None else _rows(cov, 3)
        assert v is None or v.shape == d.shape
        out = np.full(xyt.shape[0], -1, dtype=np.int32)
        self._chk(self.lib.pocs_probe_device_footprint_disc(self.h, float(radius), _dp_or_null(b), b.shape[0], _dp_or_null(d), d.shape[0],
                                                            None if v is None else _dp_or_null(v),
                                                            C.c_uint64(int(seed)), C.c_uint32(int(waypoint_word)), C.c_ulonglong(int(first)),
                                                            xyt.shape[0], xyt.ctypes.data_as(_dp), out.ctypes.data_as(C.POINTER(C.c_int))))
        return out

    def probe_device_discs(self, footprint, boxes, discs, poses):
        """Test hook: per pose (n x 3) the kinds of obstacle it touches on the device, for the caller's own footprint (dx, dy, hx, hy),
        boxes (M x 5) and discs (D x 3).  int32[n]: bit 0 = touches some box, bit 1 = touches some disc, bit 8 = the kernels' two forms
        disagree (never)."""
        fp = _arr(footprint).ravel()
        b, d, xyt = _rows(boxes, 5), _rows(discs, 3), _rows(poses, 3)
        assert fp.size == 4
        out = np.full(xyt.shape[0], -1, dtype=np.int32)
        self._chk(self.lib.pocs_probe_device_discs(self.h, fp.ctypes.data_as(_dp), _dp_or_null(b), b.shape[0], _dp_or_null(d), d.shape[0],
                                                   xyt.shape[0], xyt.ctypes.data_as(_dp), out.ctypes.data_as(C.POINTER(C.c_int))))
        return out

    def set_world(self, boxes):
        """A static world of up to MAX_WORLD_BOXES boxes, shape (M, 5) = {cx, cy, half_x, half_y, yaw}; the footprint stays as set
        (set_env, configure).  Up to 64 boxes it is set_env's world; above, a large world (include/pocs.h)."""
        b = _arr(boxes).reshape(-1, 5)
        self._chk(self.lib.pocs_set_world(self.h, b.ctypes.data_as(_dp) if b.size else None, b.shape[0]))

    def world_boxes(self):
        """Boxes of the world in force (a large world's, a static world's, a schedule's per step); 0 without a world."""
        return self.lib.pocs_get_world_boxes(self.h)

    def world_reach(self):
        """Per waypoint of the selected run (or plan) of the last GMM call under a large world: how many boxes its cull kept
        (int32 array; 0 for a waypoint that was not evaluated).  Readable after a call that failed on overflow."""
        W = max(self.path_length(), 1)
        out = np.zeros(W, dtype=np.int32)
        got = self._chk(self.lib.pocs_get_world_reach(self.h, out.ctypes.data_as(C.POINTER(C.c_int)), W))
        return out[:got]

    def set_alphas(self, a):
        a = _arr(a)
        self._chk(self.lib.pocs_set_alphas(self.h, a.ctypes.data_as(_dp), len(a)))

    def set_q(self, q):
        self._chk(self.lib.pocs_set_q(self.h, q))

    def set_landmarks(self, lm):
        lm = _arr(lm)                       # 2 x L: xs then ys
        self._chk(self.lib.pocs_set_num_landmarks(self.h, lm.shape[1]))
        self._chk(self.lib.pocs_set_landmarks(self.h, lm.ctypes.data_as(_dp), lm.shape[1]))

    def set_num_particles(self, n):
        self._chk(self.lib.pocs_set_num_particles(self.h, n))

    def set_initial_covariance(self, c):
        c = _arr(c).ravel()
        self._chk(self.lib.pocs_set_initial_covariance(self.h, c.ctypes.data_as(_dp)))

    def set_plan(self, plan):
        traj = _arr(np.asarray(plan["traj"]).T)     # by component, as setTrajectory expects
        odom = _arr(np.asarray(plan["odom"]).T)
        W = traj.shape[1]
        self._chk(self.lib.pocs_set_path_length(self.h, W))
        self._chk(self.lib.pocs_set_trajectory(self.h, traj.ctypes.data_as(_dp), W))
        self._chk(self.lib.pocs_set_odometry(self.h, odom.ctypes.data_as(_dp), W - 1))

    def set_num_gaussians(self, k):
        self._chk(self.lib.pocs_set_num_gaussians(self.h, k))

    def set_num_gmm_samples(self, n):
        self._chk(self.lib.pocs_set_num_gmm_samples(self.h, n))

    def set_seed(self, s):
        self._chk(self.lib.pocs_set_seed(self.h, s))

    def set_option(self, opt, val):
        self._chk(self.lib.pocs_set_option(self.h, opt, val))

    def set_batch(self, runs):
        """Independent GMM estimations advanced in lockstep per run_gmm_estimation / begin..end."""
        self._chk(self.lib.pocs_set_batch(self.h, runs))
        self._batch = runs

    def batch_probabilities(self):
        n = getattr(self, "_batch", 1)
        out = np.zeros(n)
        got = self._chk(self.lib.pocs_get_batch_probabilities(self.h, out.ctypes.data_as(_dp), n))
        return out[:got]

    def select_batch_run(self, run):
        """The getters (waypoint probabilities, moments, mixture state, samples ...) expose run `run` of the last batch."""
        self._chk(self.lib.pocs_select_batch_run(self.h, int(run)))

    def set_plans(self, plans):
        """Candidate plans (list of {"traj": W x 3, "odom": (W-1) x 3}): every run call then evaluates each of them once,
        in one batch; the results come in plan order and select_batch_run(p) selects plan p for the getters."""
        W, trajs, odoms = pack_plans(plans)
        if not hasattr(self, "_single_batch"):
            self._single_batch = getattr(self, "_batch", 1)
        self._chk(self.lib.pocs_set_plans(self.h, len(W), W.ctypes.data_as(C.POINTER(C.c_int)), trajs.ctypes.data_as(_dp),
                                          odoms.ctypes.data_as(_dp)))
        self._batch = len(W)

    def clear_plans(self):
        """Back to the single plan (and batch) of set_plan / set_batch."""
        self._chk(self.lib.pocs_set_plans(self.h, 0, None, None, None))
        if hasattr(self, "_single_batch"):
            self._batch = self._single_batch
            del self._single_batch

    def set_plan_risk_bound(self, bound):
        """Calls of plans on the GMM path stop a plan at the first waypoint where its running probability reaches `bound`
        (in (0, 1); >= 1.0 turns the bound off): include/pocs.h."""
        self._chk(self.lib.pocs_set_plan_risk_bound(self.h, float(bound)))

    def plan_evaluated(self):
        """Waypoints evaluated per plan in the last call of plans (int32[P]); less than the plan's length = stopped."""
        n = getattr(self, "_batch", 1)
        out = np.zeros(n, dtype=np.int32)
        got = self._chk(self.lib.pocs_get_plan_evaluated(self.h, out.ctypes.data_as(C.POINTER(C.c_int)), n))
        return out[:got]

    def set_plan_tree(self, parent, poses, odoms):
        """A tree of candidate plans: parent int[T] (parent[0] = -1, parent[n] < n), poses T x 3, odoms T x 3 (row n = the
        control of the edge parent[n] -> n; row 0 is ignored).  Every run call then evaluates each NODE once; the results
        come in node order (tree_probabilities, tree_counts) and select_tree_node(n) shows the path root -> n to the getters."""
        from .planio import check_tree
        parent, poses, odoms = check_tree(parent, poses, odoms)
        T = len(parent)
        self._chk(self.lib.pocs_set_plan_tree(self.h, T, parent.ctypes.data_as(C.POINTER(C.c_int)),
                                              _arr(poses.T).ctypes.data_as(_dp), _arr(odoms.T).ctypes.data_as(_dp)))
        self._tree_nodes = T

    def clear_plan_tree(self):
        """Back to the single plan (and batch) of set_plan / set_batch."""
        self._chk(self.lib.pocs_set_plan_tree(self.h, 0, None, None, None))
        self._tree_nodes = 0

    def tree_probabilities(self):
        """Per node, in node order: the running probability of the path root -> n of the last call on the tree."""
        T = getattr(self, "_tree_nodes", 0)
        out = np.zeros(max(T, 1))
        got = self._chk(self.lib.pocs_get_tree_probabilities(self.h, out.ctypes.data_as(_dp), T))
        return out[:got]

    def tree_evaluated(self):
        """Per node: 1 evaluated, 0 cut off below a node stopped by the risk bound (uint8[T])."""
        T = getattr(self, "_tree_nodes", 0)
        out = np.zeros(max(T, 1), dtype=np.uint8)
        got = self._chk(self.lib.pocs_get_tree_evaluated(self.h, out.ctypes.data_as(C.POINTER(C.c_ubyte)), T))
        return out[:got]

    def tree_counts(self):
        """After an MC call on the tree, per node: the particles that collided at or before n on its path (uint64[T])."""
        T = getattr(self, "_tree_nodes", 0)
        out = np.zeros(max(T, 1), dtype=np.uint64)
        got = self._chk(self.lib.pocs_mc_get_tree_counts(self.h, out.ctypes.data_as(C.POINTER(C.c_ulonglong)), T))
        return out[:got]

    def select_tree_node(self, n):
        """The getters (path length, waypoint probabilities, moments, mixture state, host chain, waypoint counts) show the
        path root -> n of the last call on the tree, as a plan of depth(n) + 1 waypoints."""
        self._chk(self.lib.pocs_select_tree_node(self.h, int(n)))

    def set_shard(self, first=-1, count=-1):
        """Evaluate global indices [first, first+count); no arguments = the whole range."""
        self._chk(self.lib.pocs_set_shard(self.h, first, count))

    def set_stream(self, stream_ptr):
        self._chk(self.lib.pocs_set_stream(self.h, stream_ptr))

    def configure(self, plan, env, params=None, K=None, N=None, seed=None):
        """Everything MCSimulation.py:154-207 pushes, from Python values."""
        from .planio import DEFAULTS
        p = dict(DEFAULTS)
        p.update(params or {})
        self.set_env(env)
        if env.get("discs") is not None:   # round obstacles beside the boxes (set_discs)
            self.set_discs(env["discs"])
        if env.get("disc_covariances") is not None:   # uncertain discs (set_disc_covariances)
            self.set_disc_covariances(env["disc_covariances"], bool(env.get("disc_noise_persistent", False)))
        if env.get("disc_hypotheses") is not None:    # prediction hypotheses: (group, weight) (set_disc_hypotheses)
            self.set_disc_hypotheses(*env["disc_hypotheses"])
        self.set_alphas(p["alphas"])
        self.set_q(p["Q"])
        self.set_landmarks(p["landmarks"])
        n = p["num_particles"] if N is None else N
        self.set_num_particles(n)
        self.set_initial_covariance(p["cov0"])
        self.set_plan(plan)
        self.set_num_gaussians(p["num_gaussians"] if K is None else K)
        self.set_num_gmm_samples(n)
        if seed is not None:
            self.set_seed(seed)

    # ---- runs -------------------------------------------------------------------------
    def run_simulation(self):
        p = C.c_double()
        self._chk(self.lib.pocs_run_simulation(self.h, C.byref(p)))
        return p.value

    def run_gmm_estimation(self):
        p = C.c_double()
        self._chk(self.lib.pocs_run_gmm_estimation(self.h, C.byref(p)))
        return p.value

    def mc_run_local(self):
        n = C.c_ulonglong()
        self._chk(self.lib.pocs_mc_run_local(self.h, C.byref(n)))
        return n.value

    def mc_batch_counts(self):
        n = getattr(self, "_batch", 1)
        out = (C.c_ulonglong * n)()
        got = self._chk(self.lib.pocs_mc_get_batch_counts(self.h, out, n))
        return [int(v) for v in out[:got]]

    def mc_waypoint_counts(self):
        """First collisions per waypoint of the selected run of the last MC call under OPT_MC_WAYPOINT_COUNTS (uint64 array):
        entry w = the shard's particles that collide at waypoint w and at no waypoint before it (include/pocs.h)."""
        W = max(self.path_length(), 1)
        out = np.zeros(W, dtype=np.uint64)
        got = self._chk(self.lib.pocs_mc_get_waypoint_counts(self.h, out.ctypes.data_as(C.POINTER(C.c_ulonglong)), W))
        return out[:got]

    def obstacle_counts(self):
        """Collision counts per waypoint and obstacle box of the current selection (run, plan or tree path) of the last call
        under OPT_OBSTACLE_COUNTS: a (E, M) uint64 array, entry [w, m] = samples at waypoint w that touch box m (GMM), or
        particles whose first collision is at w and which touch box m there (MC); include/pocs.h."""
        E = max(self.path_length(), 1)
        out = np.zeros(E * MAX_OBSTACLES, dtype=np.uint64)
        M = C.c_int(0)
        got = self._chk(self.lib.pocs_get_obstacle_counts(self.h, out.ctypes.data_as(C.POINTER(C.c_ulonglong)), out.size, C.byref(M)))
        return out[:got * M.value].reshape(got, M.value)

    def set_clearance_levels(self, d):
        """Clearance levels 0 < d[0] < d[1] < ... (at most MAX_CLEARANCE_LEVELS; an empty list turns them off): whole calls on one
        GPU then also count, per waypoint and level, the poses that pass within d of an obstacle (include/pocs.h)."""
        d = _arr(d).ravel()
        self._chk(self.lib.pocs_set_clearance_levels(self.h, d.ctypes.data_as(_dp) if d.size else None, d.size))

    def clearance_levels(self):
        """The distances in force (float64 array; empty: off)."""
        out = np.zeros(MAX_CLEARANCE_LEVELS)
        got = self._chk(self.lib.pocs_get_clearance_levels(self.h, out.ctypes.data_as(_dp), out.size))
        return out[:got]

    def clearance_counts(self):
        """Near-miss counts of the current selection (run or plan) of the last call under clearance levels: an (E, L) uint64
        array, entry [w, l] = samples at waypoint w within clearance d_l (GMM), or particles within d_l at w and at no waypoint
        before (MC); include/pocs.h."""
        E = max(self.path_length(), 1)
        out = np.zeros(E * MAX_CLEARANCE_LEVELS, dtype=np.uint64)
        L = C.c_int(0)
        got = self._chk(self.lib.pocs_get_clearance_counts(self.h, out.ctypes.data_as(C.POINTER(C.c_ulonglong)), out.size, C.byref(L)))
        return out[:got * L.value].reshape(got, L.value)

    def clearance_probabilities(self, level):
        """Per run / plan of the last call: the estimator's probability with "within d_level" in place of "collides"."""
        n = getattr(self, "_batch", 1)
        out = np.zeros(n)
        got = self._chk(self.lib.pocs_get_batch_clearance_probabilities(self.h, int(level), out.ctypes.data_as(_dp), n))
        return out[:got]

    def probe_device_clearance(self, footprint, d, boxes, poses):
        """Test hook: the device's clearance level of poses (n x 3) for a footprint (dx, dy, hx, hy), distances d and boxes (M x 5) of
        the caller's own: int32[n], -1 the footprint itself touches, else the smallest level whose grown footprint does, len(d) for none."""
        fp = _arr(footprint).ravel()
        d = _arr(d).ravel()
        b, xyt = _rows(boxes, 5), _rows(poses, 3)
        assert fp.size == 4
        out = np.full(xyt.shape[0], -99, dtype=np.int32)
        self._chk(self.lib.pocs_probe_device_clearance(self.h, fp.ctypes.data_as(_dp), _dp_or_null(d), d.size, _dp_or_null(b), b.shape[0],
                                                       xyt.shape[0], xyt.ctypes.data_as(_dp), out.ctypes.data_as(C.POINTER(C.c_int))))
        return out

    def set_footprint_parts(self, parts):
        """A compound footprint: F x (dx, dy, half_x, half_y), 1 <= F <= MAX_FOOTPRINT_PARTS; a pose touches when one of the parts
        does.  One part is set_footprint (include/pocs.h)."""
        q = _arr(parts).reshape(-1, 4)
        self._chk(self.lib.pocs_set_footprint_parts(self.h, q.ctypes.data_as(_dp) if q.size else None, q.shape[0]))

    def footprint_parts(self):
        """The parts in force: an (F, 4) float64 array (F = 1 after set_footprint)."""
        out = np.zeros((MAX_FOOTPRINT_PARTS, 4))
        got = self._chk(self.lib.pocs_get_footprint_parts(self.h, out.ctypes.data_as(_dp), MAX_FOOTPRINT_PARTS))
        return out[:got]

    def probe_footprint_parts(self, parts, boxes, poses):
        """Test hook: per pose (n x 3) the parts (F x 4) of the caller's own compound footprint that touch the caller's own boxes
        (M x 5) on the device: int32[n], bit f = part f touches, bit 8 = the kernels' two forms disagree (never)."""
        q, b, xyt = _rows(parts, 4), _rows(boxes, 5), _rows(poses, 3)
        out = np.full(xyt.shape[0], -1, dtype=np.int32)
        self._chk(self.lib.pocs_probe_device_footprint_parts(self.h, _dp_or_null(q), q.shape[0], _dp_or_null(b), b.shape[0], xyt.shape[0],
                                                             xyt.ctypes.data_as(_dp), out.ctypes.data_as(C.POINTER(C.c_int))))
        return out

    def set_regions(self, boxes, kinds=None):
        """Watched regions: up to MAX_REGIONS boxes (cx, cy, half_x, half_y, yaw_rad) with a kind each (REGION_TOUCH, the default:
        the robot's footprint touches the box; REGION_POINT: the pose's reference point lies in it); an empty list clears.  Whole MC
        calls on one GPU then also count, per waypoint and region, the never-collided particles in it (include/pocs.h)."""
        b = _arr(boxes).reshape(-1, 5)
        k = np.ascontiguousarray(np.zeros(b.shape[0]) if kinds is None else kinds, dtype=np.int32).ravel()
        assert k.size == b.shape[0]
        ip = C.POINTER(C.c_int)
        self._chk(self.lib.pocs_set_regions(self.h, b.ctypes.data_as(_dp) if b.size else None, k.ctypes.data_as(ip) if k.size else None, b.shape[0]))

    def regions(self):
        """The regions in force: (boxes (G, 5) float64, kinds int32[G]); G = 0: off."""
        b = np.zeros((MAX_REGIONS, 5))
        k = np.zeros(MAX_REGIONS, dtype=np.int32)
        got = self._chk(self.lib.pocs_get_regions(self.h, b.ctypes.data_as(_dp), k.ctypes.data_as(C.POINTER(C.c_int)), MAX_REGIONS))
        return b[:got], k[:got]

    def region_counts(self):
        """Region counts of the current selection (run or plan) of the last call under watched regions: an (E, G) uint64 array,
        entry [w, g] = the particles that have collided at no waypoint <= w and are in region g at w; include/pocs.h."""
        E = max(self.path_length(), 1)
        out = np.zeros(E * MAX_REGIONS, dtype=np.uint64)
        G = C.c_int(0)
        got = self._chk(self.lib.pocs_get_region_counts(self.h, out.ctypes.data_as(C.POINTER(C.c_ulonglong)), out.size, C.byref(G)))
        return out[:got * G.value].reshape(got, G.value)

    def region_probabilities(self, region, waypoint=-1):
        """Per run / plan of the last call: the share of the cloud that never collided and is in `region` at `waypoint` (-1: each
        plan's own last waypoint); -1.0 where the run / plan was not evaluated at that waypoint."""
        n = getattr(self, "_batch", 1)
        out = np.zeros(n)
        got = self._chk(self.lib.pocs_get_batch_region_probabilities(self.h, int(region), int(waypoint), out.ctypes.data_as(_dp), n))
        return out[:got]

    def probe_device_regions(self, footprint, boxes, kinds, poses):
        """Test hook: per pose (n x 3) the regions (G x 5, kinds[G]) of the caller's own that the device finds it in, for a footprint
        (dx, dy, hx, hy): int32[n], bit g = in region g, bit 8 + g = the kernels' two forms disagree on region g (never)."""
        fp = _arr(footprint).ravel()
        b, xyt = _rows(boxes, 5), _rows(poses, 3)
        k = np.ascontiguousarray(kinds, dtype=np.int32).ravel()
        assert fp.size == 4 and k.size == b.shape[0]
        ip = C.POINTER(C.c_int)
        out = np.full(xyt.shape[0], -1, dtype=np.int32)
        self._chk(self.lib.pocs_probe_device_regions(self.h, fp.ctypes.data_as(_dp), _dp_or_null(b),
                                                     k.ctypes.data_as(ip) if k.size else None, b.shape[0], xyt.shape[0],
                                                     xyt.ctypes.data_as(_dp), out.ctypes.data_as(ip)))
        return out

    def set_segment_checks(self, J):
        """J checks per segment, 1 <= J <= MAX_SEGMENT_CHECKS: with J >= 2 a pose also touches at a waypoint when one of J - 1 sub-poses
        on the way into it touches.  1 (the default) is every call as it has always been (include/pocs.h)."""
        self._chk(self.lib.pocs_set_segment_checks(self.h, int(J)))

    def segment_checks(self):
        """The number of checks per segment in force."""
        return self._chk(self.lib.pocs_get_segment_checks(self.h))

    def segment_counts(self):
        """Segment counts of the current selection (run or plan) of the last call under segment checks: uint64[E], entry w = the
        collisions at waypoint w that were found only between waypoints; include/pocs.h."""
        E = max(self.path_length(), 1)
        out = np.zeros(E, dtype=np.uint64)
        got = self._chk(self.lib.pocs_get_segment_counts(self.h, out.ctypes.data_as(C.POINTER(C.c_ulonglong)), out.size))
        return out[:got]

    def probe_segment(self, footprint, boxes, u, J, backward, poses):
        """Test hook: per pose (n x 3) the sub-poses of its segment that touch the caller's own boxes (M x 5) on the device, for a
        footprint (dx, dy, hx, hy), a control u (3) and J checks; backward 0: the MC form from the start pose, 1: the GMM form from the
        sample.  int32[n]: bit j (1 <= j < J) = sub-pose j touches, bit J = the end pose touches, bit 16 = the kernels' two forms
        disagree (never)."""
        fp = _arr(footprint).ravel()
        b, xyt = _rows(boxes, 5), _rows(poses, 3)
        u3 = _arr(u).ravel()
        assert fp.size == 4 and u3.size == 3
        out = np.full(xyt.shape[0], -1, dtype=np.int32)
        self._chk(self.lib.pocs_probe_device_segment(self.h, fp.ctypes.data_as(_dp), _dp_or_null(b), b.shape[0],
                                                     u3.ctypes.data_as(_dp), int(J), int(backward), xyt.shape[0],
                                                     xyt.ctypes.data_as(_dp), out.ctypes.data_as(C.POINTER(C.c_int))))
        return out

    def gmm_begin(self):
        self._chk(self.lib.pocs_gmm_begin(self.h))

    def gmm_step_local(self, w):
        self._chk(self.lib.pocs_gmm_step_local(self.h, w))

    def gmm_advance_local(self, w):
        self._chk(self.lib.pocs_gmm_advance_local(self.h, w))

    def gmm_sample_local(self, w):
        self._chk(self.lib.pocs_gmm_sample_local(self.h, w))

    def xchg_create(self, world, rank):
        """This rank's exchange buffer; returns its 64-byte IPC handle (bytes) for the peers."""
        h = C.create_string_buffer(64)
        self._chk(self.lib.pocs_xchg_create(self.h, world, rank, C.cast(h, C.c_void_p)))
        return h.raw

    def xchg_connect(self, handles):
        """handles: the 64-byte handles of rank 0 .. world-1, in rank order."""
        blob = b"".join(handles)
        buf = C.create_string_buffer(blob, len(blob))
        self._chk(self.lib.pocs_xchg_connect(self.h, C.cast(buf, C.c_void_p), len(handles)))

    def gmm_exchange_local(self, w):
        self._chk(self.lib.pocs_gmm_exchange_local(self.h, w))

    def gmm_sample_exchange_local(self, w):
        """sample(w) and exchange(w) in one launch (include/pocs.h)."""
        self._chk(self.lib.pocs_gmm_sample_exchange_local(self.h, w))

    def gmm_moments_ptr(self, w):
        return self.lib.pocs_gmm_moments_ptr(self.h, w)

    def gmm_moments_len(self):
        return self.lib.pocs_gmm_moments_len(self.h)

    def gmm_bind_moments(self, ptr, n):
        self._chk(self.lib.pocs_gmm_bind_moments(self.h, ptr, n))

    def gmm_end(self):
        p = C.c_double()
        self._chk(self.lib.pocs_gmm_end(self.h, C.byref(p)))
        return p.value

    # ---- results ----------------------------------------------------------------------
    def path_length(self):
        return self.lib.pocs_get_path_length(self.h)

    def waypoint_probabilities(self):
        W = self.path_length()
        out = np.zeros(W)
        n = self._chk(self.lib.pocs_get_waypoint_probabilities(self.h, out.ctypes.data_as(_dp), W))
        return out[:n]

    def moments(self, w, K):
        out = np.zeros(K * NMOM)
        self._chk(self.lib.pocs_get_moments(self.h, w, out.ctypes.data_as(_dp), out.size))
        return out.reshape(K, NMOM)

    def gmm_state(self, w, K):
        m, c, wt, al = np.zeros((K, 3)), np.zeros((K, 9)), np.zeros(K), np.zeros(K)
        self._chk(self.lib.pocs_get_gmm_state(self.h, w, m.ctypes.data_as(_dp), c.ctypes.data_as(_dp),
                                              wt.ctypes.data_as(_dp), al.ctypes.data_as(_dp)))
        return m, c.reshape(K, 3, 3), wt, al

    def gmm_state_raw(self, w, K):
        """K x 16 rows [mean(3) cov(9) weight alive 0 0] -- the layout the oracle uses too."""
        m, c, wt, al = self.gmm_state(w, K)
        s = np.zeros((K, 16))
        s[:, 0:3], s[:, 3:12], s[:, 12], s[:, 13] = m, c.reshape(K, 9), wt, al
        return s

    def host_chain(self, L):
        n = max(self.path_length() - 1, 0)
        a, no, z = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, L))
        mu, cov = np.zeros((n, 3)), np.zeros((n, 9))
        self._chk(self.lib.pocs_get_host_chain(self.h, *(x.ctypes.data_as(_dp) for x in (a, no, z, mu, cov))))
        return dict(applied=a, noisy=no, z=z, mu=mu, cov=cov)

    def gmm_samples(self, n):
        xyz = np.zeros((n, 3))
        flags = np.zeros(n, np.int16)
        got = self._chk(self.lib.pocs_copy_gmm_samples(self.h, xyz.ctypes.data_as(_dp),
                                                       flags.ctypes.data_as(C.POINTER(C.c_int16)), n))
        return xyz[:got], flags[:got]

    def particles(self, n):
        xyz = np.zeros((n, 3))
        hits = np.zeros(n, np.uint32)
        got = self._chk(self.lib.pocs_copy_particles(self.h, xyz.ctypes.data_as(_dp),
                                                     hits.ctypes.data_as(C.POINTER(C.c_uint32)), n))
        return xyz[:got], hits[:got]

    def copy_bandwidth(self, nbytes=1 << 30):
        """GB/s (read + written) of a plain streaming copy of nbytes on this GPU."""
        g = C.c_double()
        self._chk(self.lib.pocs_measure_copy_bandwidth(self.h, nbytes, C.byref(g)))
        return g.value

    def fill_bandwidth(self, nbytes=1 << 30):
        """GB/s written by a plain streaming fill of nbytes on this GPU."""
        g = C.c_double()
        self._chk(self.lib.pocs_measure_fill_bandwidth(self.h, nbytes, C.byref(g)))
        return g.value

    def sequence_time(self):
        """(ms from the first sampling launch to the end of the last, sub-batches in flight side by side) of the last
        whole-run GMM call under OPT_PROFILE."""
        ms, g = C.c_double(0.0), C.c_int(1)
        self._chk(self.lib.pocs_get_sequence_time(self.h, C.byref(ms), C.byref(g)))
        return ms.value, g.value

    def exchange_wait_us(self):
        """(min, median, max) over the (run, waypoint) pairs of the last sharded begin..end sequence of how long the
        closers waited for the other ranks' moments, in microseconds (the library's own exchange only)."""
        v = (C.c_double * 3)()
        self._chk(self.lib.pocs_get_exchange_wait(self.h, v))
        return v[0], v[1], v[2]

    def probe_device_math(self, radius_words, angle_words, headings):
        """Test hook: the device's table-driven sampler functions on chosen inputs -> (z0, z1, sin, cos, radius^2) arrays."""
        wr = np.ascontiguousarray(radius_words, dtype=np.uint32)
        wa = np.ascontiguousarray(angle_words, dtype=np.uint32)
        x = np.ascontiguousarray(headings, dtype=np.float64)
        n = len(wr)
        assert len(wa) == n and len(x) == n
        out = [np.empty(n) for _ in range(5)]
        u32 = C.POINTER(C.c_uint32)
        self._chk(self.lib.pocs_probe_device_math(self.h, n, wr.ctypes.data_as(u32), wa.ctypes.data_as(u32), x.ctypes.data_as(_dp),
                                                  *[o.ctypes.data_as(_dp) for o in out]))
        return tuple(out)

    def probe_device_radius_roots(self, first_word, count):
        """Test hook: the sampler's short square root of the Box-Muller radius against the correctly rounded one on the device,
        for the words first_word .. first_word + count - 1 -> (words whose roots differ, the smallest of them or 0)."""
        first, count = int(first_word), int(count)
        if not (0 <= first < 1 << 32 and 0 <= count <= 1 << 32):      # (ctypes would wrap them silently)
            raise PocsError(-1, "probe_device_radius_roots: a range outside the 32-bit words")
        bad, word = C.c_ulonglong(0), C.c_uint32(0)
        self._chk(self.lib.pocs_probe_device_radius_roots(self.h, first, count, C.byref(bad), C.byref(word)))
        return bad.value, word.value

    def probe_device_collide(self, params, poses):
        """Test hook: the device's collision test and the sampling kernel's obstacle cull on chosen inputs, against the
        context's world (set_env).  params: K x 12 sampler parameters of a mixture (mean[3], L00 L10 L11 L20 L21 L22, ...);
        poses: n x 3 (x, y, theta).  -> (flag_full, flag_pair, flag_pair_eager: int32[n]; kept: nkeep x 8 records)."""
        par = _arr(params).reshape(-1, 12)
        xyt = _arr(poses).reshape(-1, 3)
        K, n = par.shape[0], xyt.shape[0]
        flags = [np.full(n, -1, dtype=np.int32) for _ in range(3)]
        nkeep = C.c_int(-1)
        kept = np.zeros((64, 8))
        ip = C.POINTER(C.c_int)
        self._chk(self.lib.pocs_probe_device_collide(self.h, K, par.ctypes.data_as(_dp), n, xyt.ctypes.data_as(_dp),
                                                     *[f.ctypes.data_as(ip) for f in flags], C.byref(nkeep), kept.ctypes.data_as(_dp)))
        return flags[0], flags[1], flags[2], kept[:nkeep.value].copy()

    def probe_device_counts(self, K, weights, alive, seeds, waypoints, n_total):
        """Test hook: the device's component counts of a waypoint on chosen inputs, n cases in one launch.  K: int[n], the components
        of each case (1 .. 8); weights, alive: n x 8 (raw weights >= 0 and alive flags, case i uses the first K[i]); seeds (uint64),
        waypoints (uint32), n_total (int64, 1 .. 2^53): n each.  -> n x 8 cumulative counts (float64), zeros behind a case's K."""
        k = np.ascontiguousarray(K, dtype=np.int32).ravel()
        n = len(k)
        w, a = _arr(weights), _arr(alive)
        s = np.ascontiguousarray(seeds, dtype=np.uint64).ravel()
        wp = np.ascontiguousarray(waypoints, dtype=np.uint32).ravel()
        nt = np.ascontiguousarray(n_total, dtype=np.int64).ravel()
        if w.shape != (n, 8) or a.shape != (n, 8) or not (len(s) == len(wp) == len(nt) == n):
            raise ValueError("%d cases: weights and alive are n x 8, seeds, waypoints and n_total have n entries" % n)
        out = np.full((n, 8), -1.0)
        self._chk(self.lib.pocs_probe_device_counts(self.h, n, k.ctypes.data_as(C.POINTER(C.c_int)), w.ctypes.data_as(_dp), a.ctypes.data_as(_dp),
                                                    s.ctypes.data_as(C.POINTER(C.c_uint64)), wp.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                    nt.ctypes.data_as(C.POINTER(C.c_longlong)), out.ctypes.data_as(_dp)))
        return out

    def graph_captures(self):
        """(gmm, mc): how often the whole GMM call's and the MC call's launches have been captured into a graph so far."""
        g, m = C.c_longlong(), C.c_longlong()
        self._chk(self.lib.pocs_get_graph_captures(self.h, C.byref(g), C.byref(m)))
        return g.value, m.value

    def kernel_time(self):
        ms, n = C.c_double(), C.c_longlong()
        self._chk(self.lib.pocs_get_kernel_time(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value
