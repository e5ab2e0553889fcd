"""ctypes binding of include/graphslam.h (libgraphslam_hip.so).

This is plumbing above the C-ABI: the product is the HIP library.  There is no CPU fallback: if the
shared library is missing or no gfx950 device is usable, calls raise.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import cheader

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_PATH = os.environ.get("GS_LIB") or os.path.join(CSRC, "libgraphslam_hip.so")    # GS_LIB: A/B builds of the same library (tuning)
HEADER = os.path.join(os.path.dirname(HERE), "include", "graphslam.h")
DEBUG_HEADER = os.path.join(os.path.dirname(HERE), "include", "graphslam_debug.h")     # tuning / fault injection / timestamps: not the drop-in boundary

# The headers are the one statement of the ABI on this side too: every constant, struct and prototype below is read from them (cheader.py)
ABI = cheader.Abi()
for _h in (HEADER, DEBUG_HEADER):
    with open(_h) as _f:
        ABI.read(_f.read(), _h)

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_int64)


def _defines(prefix):
    """the header's #define <prefix>* integers by lower-case name, in the header's order"""
    return {k[len(prefix):].lower(): v for k, v in ABI.defines.items() if k.startswith(prefix)}


GS_OK = ABI.defines["GS_OK"]
ERRORS = {v: "GS_ERR_" + k.upper() for k, v in _defines("GS_ERR_").items()}
ROBUST_KERNELS = _defines("GS_ROBUST_")                     # gs_set_robust_kernel: GS_ROBUST_* / GS_EDGE_* by name
EDGE_KINDS = _defines("GS_EDGE_")
DOGLEG_KINDS = tuple(k.upper() for k in sorted(_defines("GS_DOGLEG_"), key=_defines("GS_DOGLEG_").get))    # ("GN", "SD", "DL")
NN_FRAME_MAX, LOC_ITER_MAX, RELOC_SEED_MAX, FOLLOW_HYP_MAX, CAND_MAX, DUP_MAP_MAX = (
    ABI.defines["GS_" + k] for k in ("NN_FRAME_MAX", "LOC_ITER_MAX", "RELOC_SEED_MAX", "FOLLOW_HYP_MAX", "CAND_MAX", "DUP_MAP_MAX"))


class GsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (ERRORS.get(code, "GS_ERR"), code, msg))
        self.code = code


# ---- the structs: ctypes mirrors for the ones passed by pointer, numpy records for the ones that come in arrays
Config = ABI.structure("Config", "gs_config")
ShellMsg = ABI.structure("ShellMsg", "gs_shell_msg")
DebugOptions = ABI.structure("DebugOptions", "gs_debug_options")    # every tuning switch of a handle (include/graphslam_debug.h)
PlanInfo = ABI.structure("PlanInfo", "gs_plan_info")
LmParams = ABI.structure("LmParams", "gs_lm_params")
DoglegParams = ABI.structure("DoglegParams", "gs_dogleg_params")
NnParams = ABI.structure("NnParams", "gs_nn_params")                # the gate and the noise model of the covariance-gated association
JcParams = ABI.structure("JcParams", "gs_jc_params")                # the joint compatibility test's gate per number of kept pairs
LocParams = ABI.structure("LocParams", "gs_loc_params")             # the iteration limit and the stop tolerances of frame localisation
RelocParams = ABI.structure("RelocParams", "gs_reloc_params")       # the seeds, the tolerances and what counts as a different pose
FollowParams = ABI.structure("FollowParams", "gs_follow_params")    # when a fit is accepted, a hypothesis lost, two have become one
CandParams = ABI.structure("CandParams", "gs_cand_params")          # when a candidate is confirmed or retired, where one may spawn
DupParams = ABI.structure("DupParams", "gs_dup_params")             # which cone pairs of a map count as twins
FOLLOW_STATE, FOLLOW_STEP = ABI.dtype("gs_follow_state"), ABI.dtype("gs_follow_step")
CAND, CAND_STEP, DUP_INFO = ABI.dtype("gs_cand"), ABI.dtype("gs_cand_step"), ABI.dtype("gs_dup_info")

# switches applied to every handle this process creates through the binding (tests: conftest sets grow_min_poses = 0)
DEFAULT_DEBUG = {}


@ABI.mirror("gs_stats")
class Stats(C.Structure):
    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


@ABI.mirror("gs_marginals_info")
class MarginalsInfo(C.Structure):
    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


@ABI.mirror("gs_lm_info", rename={"lambda": "lambda_"})          # (a Python keyword: the one field not under its header name)
class LmInfo(C.Structure):
    """gs_lm_info: counters of a gs_optimize_lm call and its per-iteration history (the first iterations only)"""

    def as_dict(self):
        """scalars as they are; the histories as arrays cut to the iterations that ran (one more than accepted after a terminate)"""
        n = min(self.iterations + (1 if self.terminated else 0), len(self.chi2))
        o = {k: getattr(self, k) for k in ("iterations", "trials", "rejected", "terminated", "lambda_initial", "lambda_final")}
        o["chi2"] = np.array(self.chi2[:n]); o["lambda"] = np.array(self.lambda_[:n]); o["n_trials"] = np.array(self.n_trials[:n], dtype=np.int32)
        return o


@ABI.mirror("gs_dogleg_info")
class DoglegInfo(C.Structure):
    """gs_dogleg_info: counters of a gs_optimize_dogleg call and its per-iteration history (the first iterations only)"""

    def as_dict(self):
        """scalars as they are; the histories as arrays cut to the iterations that ran (one more than accepted after a terminate)"""
        n = min(self.iterations + (1 if self.terminated else 0), len(self.chi2))
        o = {k: getattr(self, k) for k in ("iterations", "trials", "rejected", "terminated", "n_gn", "n_sd", "n_dl", "delta_initial", "delta_final")}
        o["chi2"] = np.array(self.chi2[:n]); o["delta"] = np.array(self.delta[:n])
        o["n_trials"] = np.array(self.n_trials[:n], dtype=np.int32); o["step_kind"] = np.array(self.step_kind[:n], dtype=np.int32)
        return o


# A struct of parameters is the library's defaults with the named fields replaced.  Per struct: the fields that may NOT be named (every
# other field of the header's struct may), and what naming one of those or an unknown one raises.
_PARAMS = {"gs_nn_params": ((), KeyError),
           "gs_loc_params": (("struct_size",), AttributeError),
           "gs_reloc_params": (("reserved",), AttributeError),
           "gs_follow_params": (("struct_size", "reserved"), AttributeError),
           "gs_cand_params": (("struct_size", "reserved"), AttributeError),
           "gs_dup_params": (("struct_size", "reserved"), AttributeError),
           "gs_lm_params": (("struct_size",), AttributeError),
           "gs_dogleg_params": (("struct_size",), AttributeError)}


def _params(cname, kw):
    fixed, error = _PARAMS[cname]
    p = ABI.mirrors[cname](); L = lib()
    rc = getattr(L, cname + "_default")(C.byref(p))
    if rc != GS_OK:
        raise GsError(rc, (L.gs_last_error() or b"").decode())
    for k, v in kw.items():
        if k == "max_trials":                               # short for max_trials_after_failure (gs_lm_params, gs_dogleg_params)
            k = "max_trials_after_failure"
        if k in fixed or k not in dict(p._fields_):
            raise error("%s has no field %r" % (cname, k))
        setattr(p, k, v)
    return p


def nn_params(**kw): return _params("gs_nn_params", kw)
def loc_params(**kw): return _params("gs_loc_params", kw)
def reloc_params(**kw): return _params("gs_reloc_params", kw)
def follow_params(**kw): return _params("gs_follow_params", kw)
def cand_params(**kw): return _params("gs_cand_params", kw)
def dup_params(**kw): return _params("gs_dup_params", kw)
def lm_params(**kw): return _params("gs_lm_params", kw)             # max_trials: short for max_trials_after_failure
def dogleg_params(**kw): return _params("gs_dogleg_params", kw)     # the same


def jc_params(confidence=None):
    """the library's gs_jc_params: the defaults (0.95), or the table of the given confidence"""
    p = JcParams(); L = lib()
    rc = L.gs_jc_params_default(C.byref(p)) if confidence is None else L.gs_jc_params_set_confidence(C.byref(p), float(confidence))
    if rc != GS_OK:
        raise GsError(rc, (L.gs_last_error() or b"").decode())
    return p


# The per-frame records of the joint test and of localisation: (the record as a dict of arrays, its C arguments in the header's order)
def _jc_record(n_frames):
    r = {"joint_d2": np.zeros(n_frames), "n_kept": np.zeros(n_frames, dtype=np.int32), "n_dropped": np.zeros(n_frames, dtype=np.int32),
         "n_untestable": np.zeros(n_frames, dtype=np.int32), "delta": np.zeros((n_frames, 3))}
    return r, (_d(r["joint_d2"]), _i(r["n_kept"]), _i(r["n_dropped"]), _i(r["n_untestable"]), _d(r["delta"]))


def _loc_record(n_frames):
    r = {"pose": np.zeros((n_frames, 3)), "cov": np.zeros((n_frames, 9)), "chi2": np.zeros(n_frames), "n_pairs": np.zeros(n_frames, dtype=np.int32),
         "iterations": np.zeros(n_frames, dtype=np.int32), "status": np.zeros(n_frames, dtype=np.int32)}
    return r, (_d(r["pose"]), _d(r["cov"]), _d(r["chi2"]), _i(r["n_pairs"]), _i(r["iterations"]), _i(r["status"]))


def _reloc_record(n_frames):
    return {"pose": np.zeros((n_frames, 3)), "count": np.zeros(n_frames, dtype=np.int32), "cost": np.zeros(n_frames), "seed": np.zeros((n_frames, 4), dtype=np.int32),
            "second_count": np.zeros(n_frames, dtype=np.int32), "second_pose": np.zeros((n_frames, 3)), "n_seeds": np.zeros(n_frames, dtype=np.int64),
            "status": np.zeros(n_frames, dtype=np.int32)}


def _reloc_record_args(r, second):
    """the C arguments of a search record; second=False: NULL for the runner-up's fields, which skips its pass"""
    return (_d(r["pose"]), _i(r["count"]), _d(r["cost"]), _i(r["seed"]), _i(r["second_count"]) if second else None, _d(r["second_pose"]) if second else None,
            r["n_seeds"].ctypes.data_as(_lp), _i(r["status"]))


# The prototypes of the headers under the rules of cheader.py, except two parameters: the 128-byte unique id of RCCL is declared void * and
# passed as a Python bytes object / string buffer
PROTOTYPE_OVERRIDES = {("gs_dist_unique_id", "out_128_bytes"): C.c_char_p, ("gs_dist_comm_init", "unique_id_128_bytes"): C.c_char_p}
PROTOTYPES = {fn: ABI.prototype(fn, PROTOTYPE_OVERRIDES) for fn in ABI.protos}


def declared_symbols(debug=True):
    """Every function name include/graphslam.h (and, debug=True, include/graphslam_debug.h) declares."""
    return sorted(fn for fn, (origin, _, _) in ABI.protos.items() if debug or origin == HEADER)


def build(force=False):
    """Compile libgraphslam_hip.so for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j4"]
    if force:
        subprocess.check_call(["make", "-C", CSRC, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)


_lib = None


def lib():
    """Load the HIP library and give every declared function it exports the header's prototype (a library loaded through GS_LIB may be an
    older build that lacks some).  Raises if it has not been built: there is no fallback path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libgraphslam_hip.so is missing (run __graft_entry__.build()); "
                               "the GraphSLAM back-end has no CPU fallback")
        L = C.CDLL(LIB_PATH)
        for fn, (restype, argtypes) in PROTOTYPES.items():
            f = getattr(L, fn, None)
            if f is not None:
                f.restype = restype; f.argtypes = argtypes
        _lib = L
    return _lib


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a if shape is None else a.reshape(shape)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _d(a):
    return a.ctypes.data_as(_dp)


def _i(a):
    return a.ctypes.data_as(_ip)


def _vp(a):
    """an array of records, for a parameter declared as a pointer to the record struct"""
    return a.ctypes.data_as(C.c_void_p)


def _ptr(a):
    """the address of an optional DeviceArray"""
    return None if a is None else a.ptr


def default_config(**kw):
    cfg = Config()
    lib().gs_config_default(C.byref(cfg))
    for k, v in kw.items():
        if k.endswith("_robust_kernel"):
            v = ROBUST_KERNELS.get(v, v)
        setattr(cfg, k, v)
    return cfg


_hip = None


def hip_runtime():
    """libamdhip64 (the runtime the library itself uses), for callers that keep their OWN buffers in device memory (gs_associate_resident,
    gs_dist_set_exchange_buffer): tests and bench.py — a C++ consumer calls hipMalloc / hipMemcpy itself."""
    global _hip
    if _hip is None:
        lib()                                               # the library has loaded the runtime already
        H = C.CDLL("libamdhip64.so")
        H.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]; H.hipFree.argtypes = [C.c_void_p]
        H.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip = H
    return _hip


class DeviceArray:
    """A caller-owned array in device memory (hipMalloc + hipMemcpy), e.g. the observations of gs_associate_resident."""

    def __init__(self, host=None, nbytes=None):
        H = hip_runtime()
        self.host = None if host is None else np.ascontiguousarray(host)
        self.nbytes = int(nbytes if nbytes is not None else self.host.nbytes)
        p = C.c_void_p()
        if H.hipMalloc(C.byref(p), max(self.nbytes, 8)) != 0:
            raise RuntimeError("hipMalloc failed")
        self.ptr = p
        if self.host is not None and self.nbytes:
            if H.hipMemcpy(self.ptr, self.host.ctypes.data_as(C.c_void_p), self.nbytes, 1) != 0:
                raise RuntimeError("hipMemcpy (host to device) failed")

    def to_host(self, dtype, count):
        out = np.zeros(count, dtype=dtype)
        if hip_runtime().hipMemcpy(out.ctypes.data_as(C.c_void_p), self.ptr, out.nbytes, 2) != 0:
            raise RuntimeError("hipMemcpy (device to host) failed")
        return out

    def free(self):
        if getattr(self, "ptr", None):
            hip_runtime().hipFree(self.ptr); self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def dist_unique_id():
    """ncclGetUniqueId through the library (128 bytes): made by one rank, handed to the others by whatever channel they share."""
    buf = C.create_string_buffer(128)
    rc = lib().gs_dist_unique_id(buf)
    if rc < 0:
        raise GsError(rc, (lib().gs_last_error() or b"").decode())
    return buf.raw


def device_count():
    return int(lib().gs_device_count())


class Graph:
    """Mirror of the calls Slam makes on g2o::SparseOptimizer (reference src/slam.cpp:53-65,433-484,525-550)."""

    def __init__(self, cfg=None, _handle=None, debug=None, **kw):
        self.L = lib()
        self._owned = _handle is None
        if _handle is not None:
            self.h = C.c_void_p(_handle)
            return
        if cfg is None:
            cfg = default_config(**kw)
        h = C.c_void_p()
        self._check(self.L.gs_create(C.byref(cfg), C.byref(h)))
        self.h = h
        if DEFAULT_DEBUG or debug:
            self.set_debug(**dict(DEFAULT_DEBUG, **(debug or {})))

    # ---- tuning switches (include/graphslam_debug.h)
    def debug_options(self):
        o = DebugOptions(); self._check(self.L.gs_debug_get_options(self.h, C.byref(o))); return o

    def set_debug(self, **kw):
        """gs_debug_set_options: change the named switches of this handle, keep the others."""
        o = self.debug_options()
        for k, v in kw.items():
            if not hasattr(o, k):
                raise AttributeError("gs_debug_options has no field %r" % k)
            setattr(o, k, int(v))
        self._check(self.L.gs_debug_set_options(self.h, C.byref(o)))

    def _check(self, rc):
        if rc < 0:
            raise GsError(rc, (self.L.gs_last_error() or b"").decode())
        return rc

    def close(self):
        if getattr(self, "h", None) and self._owned:
            self.L.gs_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- construction
    def add_pose(self, pid, est):
        e = _f64(est); self._check(self.L.gs_add_pose(self.h, int(pid), _d(e)))

    def add_landmark(self, lid, est):
        e = _f64(est); self._check(self.L.gs_add_landmark(self.h, int(lid), _d(e)))

    def add_odometry_edge(self, i, j, z, info):
        z = _f64(z); info = _f64(info); self._check(self.L.gs_add_odometry_edge(self.h, int(i), int(j), _d(z), _d(info)))

    def add_observation_edge(self, p, l, z, info):
        z = _f64(z); info = _f64(info); self._check(self.L.gs_add_observation_edge(self.h, int(p), int(l), _d(z), _d(info)))

    def add_poses(self, ids, est):
        ids = _i32(ids); est = _f64(est); self._check(self.L.gs_add_poses(self.h, len(ids), _i(ids), _d(est)))

    def add_landmarks(self, ids, est):
        ids = _i32(ids); est = _f64(est); self._check(self.L.gs_add_landmarks(self.h, len(ids), _i(ids), _d(est)))

    def add_odometry_edges(self, i, j, z, info=None):
        i = _i32(i); j = _i32(j); z = _f64(z)
        ip = _d(_f64(info)) if info is not None else None
        if info is not None:
            info = _f64(info); ip = _d(info)
        self._check(self.L.gs_add_odometry_edges(self.h, len(i), _i(i), _i(j), _d(z), ip))

    def add_observation_edges(self, p, l, z, info=None):
        p = _i32(p); l = _i32(l); z = _f64(z); ip = None
        if info is not None:
            info = _f64(info); ip = _d(info)
        self._check(self.L.gs_add_observation_edges(self.h, len(p), _i(p), _i(l), _d(z), ip))

    def set_fixed_pose(self, pid, fixed=True):
        self._check(self.L.gs_set_fixed_pose(self.h, int(pid), int(fixed)))

    def set_fixed_landmark(self, lid, fixed=True):
        self._check(self.L.gs_set_fixed_landmark(self.h, int(lid), int(fixed)))

    def set_pose_estimate(self, pid, est):
        e = _f64(est); self._check(self.L.gs_set_pose_estimate(self.h, int(pid), _d(e)))

    def set_landmark_estimate(self, lid, est):
        e = _f64(est); self._check(self.L.gs_set_landmark_estimate(self.h, int(lid), _d(e)))

    def clear(self):
        self._check(self.L.gs_clear(self.h))

    # ---- read-back
    @property
    def n_poses(self): return self._check(self.L.gs_num_poses(self.h))
    @property
    def n_landmarks(self): return self._check(self.L.gs_num_landmarks(self.h))
    @property
    def n_pp(self): return self._check(self.L.gs_num_odometry_edges(self.h))
    @property
    def n_pl(self): return self._check(self.L.gs_num_observation_edges(self.h))

    def get_pose(self, pid):
        o = np.zeros(3); self._check(self.L.gs_get_pose(self.h, int(pid), _d(o))); return o

    def get_landmark(self, lid):
        o = np.zeros(2); self._check(self.L.gs_get_landmark(self.h, int(lid), _d(o))); return o

    def poses(self):
        n = self.n_poses; o = np.zeros((n, 3)); self._check(self.L.gs_get_poses(self.h, n, None, _d(o))); return o

    def landmarks(self):
        n = self.n_landmarks; o = np.zeros((n, 2)); self._check(self.L.gs_get_landmarks(self.h, n, None, _d(o))); return o

    # ---- optimisation
    def initialize_optimization(self):
        self._check(self.L.gs_initialize_optimization(self.h))

    def optimize(self, iterations=10, stats=True):
        if not stats:                                       # the way Slam calls it (csrc/gs_slam.cpp: no statistics asked for, no chi2 pass behind the iterations)
            return self._check(self.L.gs_optimize(self.h, int(iterations), None)), None
        st = Stats(); st.struct_size = C.sizeof(Stats)
        done = self._check(self.L.gs_optimize(self.h, int(iterations), C.byref(st)))
        return done, st

    def optimize_until(self, max_iterations, rel_chi2_tol):
        st = Stats(); st.struct_size = C.sizeof(Stats)
        done = self._check(self.L.gs_optimize_until(self.h, int(max_iterations), float(rel_chi2_tol), C.byref(st)))
        return done, st

    def _optimize_steps(self, entry, p, info, iterations):
        """an entry point of a step-control method: (accepted iterations, Stats, its info struct as a dict)"""
        st = Stats(); st.struct_size = C.sizeof(Stats)
        info.struct_size = C.sizeof(info)
        done = self._check(entry(self.h, int(iterations), C.byref(p), C.byref(st), C.byref(info)))
        return done, st, info.as_dict()

    def optimize_lm(self, iterations=10, **params):
        """gs_optimize_lm (Levenberg-Marquardt, g2o's rule): params = fields of gs_lm_params (max_trials_after_failure or max_trials,
        initial_lambda, tau); returns (accepted iterations, Stats, gs_lm_info as a dict)"""
        return self._optimize_steps(self.L.gs_optimize_lm, lm_params(**params), LmInfo(), iterations)

    def optimize_dogleg(self, iterations=10, **params):
        """gs_optimize_dogleg (Powell's dogleg, g2o's rule): params = fields of gs_dogleg_params (max_trials_after_failure or max_trials,
        initial_delta); returns (accepted iterations, Stats, gs_dogleg_info as a dict)"""
        return self._optimize_steps(self.L.gs_optimize_dogleg, dogleg_params(**params), DoglegInfo(), iterations)

    def debug_fail_at_iteration(self, k, code=1):
        self._check(self.L.gs_debug_fail_at_iteration(self.h, int(k), int(code)))

    def iterate(self):
        return self._check(self.L.gs_iterate(self.h))

    def synchronize(self):
        self._check(self.L.gs_stream_synchronize(self.h))

    def sync_estimates(self):
        self._check(self.L.gs_sync_estimates(self.h))

    def chi2(self):
        o = C.c_double(); self._check(self.L.gs_chi2(self.h, C.byref(o))); return o.value

    def stats(self):
        st = Stats(); self._check(self.L.gs_get_stats(self.h, C.byref(st))); return st

    def set_stream(self, stream_ptr):
        self._check(self.L.gs_set_stream(self.h, C.c_void_p(stream_ptr)))

    # ---- measurement / parity hooks
    def linearize(self):
        self._check(self.L.gs_linearize(self.h))

    def time_linearize(self, reps):
        return self._timed(self.L.gs_time_linearize, [self.h], reps)

    def linearize_bytes(self):
        return int(self.L.gs_linearize_bytes(self.h))

    def debug_front_times(self):
        """[2, n_fronts] completion times (100 MHz ticks) of the last factor / backward-solve launches (F3_DONE_TS builds)."""
        n = self.stats().n_fronts; buf = (C.c_int64 * (2 * n))()
        self._check(self.L.gs_debug_front_times(self.h, buf, 2 * n)); return np.array(buf[:], dtype=np.int64).reshape(2, n)

    def debug_timestamps(self):
        """100 MHz phase timestamps of one front (tuning aid, see include/graphslam.h gs_debug_timestamps)."""
        buf = (C.c_int64 * 64)(); self._check(self.L.gs_debug_timestamps(self.h, buf)); return np.array(buf[:], dtype=np.int64)

    def time_iterations(self, reps):
        st = Stats(); self._check(self.L.gs_time_iterations(self.h, int(reps), C.byref(st))); return st

    def export_system(self):
        """Block-sparse H and b of the last linearisation, edge arrays re-ordered to INSERTION order."""
        N, M, Epp, Epl = self.n_poses, self.n_landmarks, self.n_pp, self.n_pl
        o = dict(Hpp_diag=np.zeros((N, 9)), Hll_diag=np.zeros((M, 4)), Hpp_off=np.zeros((Epp, 9)),
                 Hpl=np.zeros((Epl, 6)), b_pose=np.zeros((N, 3)), b_lm=np.zeros((M, 2)))
        ppo = np.zeros(Epp, dtype=np.int32); plo = np.zeros(Epl, dtype=np.int32)
        self._check(self.L.gs_export_system(self.h, _d(o["Hpp_diag"]), _d(o["Hll_diag"]), _d(o["Hpp_off"]),
                                            _d(o["Hpl"]), _d(o["b_pose"]), _d(o["b_lm"]), _i(ppo), _i(plo)))
        hpp = np.zeros_like(o["Hpp_off"]); hpp[ppo] = o["Hpp_off"]; o["Hpp_off"] = hpp
        hpl = np.zeros_like(o["Hpl"]); hpl[plo] = o["Hpl"]; o["Hpl"] = hpl
        return o

    def export_delta(self):
        dp = np.zeros((self.n_poses, 3)); dl = np.zeros((self.n_landmarks, 2))
        self._check(self.L.gs_export_delta(self.h, _d(dp), _d(dl))); return dp, dl

    def multiply_hessian(self, v_pose, v_lm):
        """gs_multiply_hessian: (H v) per pose [N,3] and per landmark [M,2], H the system of the last linearisation on the device"""
        vp = _f64(v_pose, (self.n_poses, 3)); vl = _f64(v_lm, (self.n_landmarks, 2))
        yp = np.zeros_like(vp); yl = np.zeros_like(vl)
        self._check(self.L.gs_multiply_hessian(self.h, _d(vp), _d(vl), _d(yp), _d(yl))); return yp, yl

    # ---- marginal covariances (gs_compute_marginals: selected inversion of the factor at the current estimates)
    def compute_marginals(self):
        """Sigma = H^-1 on the pattern of the factor at the current estimates; returns the gs_marginals_info as a dict"""
        info = MarginalsInfo(); self._check(self.L.gs_compute_marginals(self.h, C.byref(info))); return info.as_dict()

    def pose_covariances(self):
        """[N,3,3] in the order of poses() (zeros for fixed poses)"""
        n = self.n_poses; out = np.zeros((n, 3, 3)); self._check(self.L.gs_get_pose_covariances(self.h, n, None, _d(out))); return out

    def landmark_covariances(self):
        """[M,2,2] in the order of landmarks()"""
        n = self.n_landmarks; out = np.zeros((n, 2, 2)); self._check(self.L.gs_get_landmark_covariances(self.h, n, None, _d(out))); return out

    def odometry_edge_covariances(self):
        """[E,3,3] Sigma(x_i, x_j) per odometry edge, insertion order"""
        n = self.n_pp; out = np.zeros((n, 3, 3)); self._check(self.L.gs_get_odometry_edge_covariances(self.h, n, _d(out))); return out

    def observation_edge_covariances(self):
        """[E,3,2] Sigma(x_p, l) per observation edge, insertion order"""
        n = self.n_pl; out = np.zeros((n, 3, 2)); self._check(self.L.gs_get_observation_edge_covariances(self.h, n, _d(out))); return out

    def covariance_block(self, kind_a, id_a, kind_b, id_b):
        """Sigma(a, b), kind 0 pose / 1 landmark (or "pose" / "landmark"); GsError GS_ERR_OUT_OF_PATTERN outside the factor's pattern"""
        ka = {"pose": 0, "landmark": 1}.get(kind_a, kind_a); kb = {"pose": 0, "landmark": 1}.get(kind_b, kind_b)
        out = np.zeros((3 if ka == 0 else 2, 3 if kb == 0 else 2))
        self._check(self.L.gs_get_covariance_block(self.h, int(ka), int(id_a), int(kb), int(id_b), _d(out))); return out

    # ---- robust kernels (gs_set_robust_kernel: per edge kind on the handle)
    def set_robust_kernel(self, kind, kernel, delta=1.0):
        """kind "odometry" / "observation", kernel "none" / "huber" / "cauchy" (or the GS_EDGE_* / GS_ROBUST_* numbers); delta in units of sqrt(e^T Omega e)"""
        self._check(self.L.gs_set_robust_kernel(self.h, int(EDGE_KINDS.get(kind, kind)), int(ROBUST_KERNELS.get(kernel, kernel)), float(delta)))

    def robust_kernel(self, kind):
        """(kernel name, delta) of the edge kind"""
        k = C.c_int32(); d = C.c_double()
        self._check(self.L.gs_get_robust_kernel(self.h, int(EDGE_KINDS.get(kind, kind)), C.byref(k), C.byref(d)))
        return {v: n for n, v in ROBUST_KERNELS.items()}.get(k.value, k.value), d.value

    def edge_chi2(self, kind):
        """(chi2, weight): s = e^T Omega e and rho'(s) of every edge of the kind at the current estimates, insertion order"""
        kd = int(EDGE_KINDS.get(kind, kind))
        n = self.n_pp if kd == 0 else self.n_pl
        s = np.zeros(n); w = np.zeros(n)
        self._check(self.L.gs_get_edge_chi2(self.h, kd, n, _d(s), _d(w))); return s, w

    # ---- prior edges (gs_add_*_prior: unary edges on a pose or a landmark; information full, row-major, required)
    def add_pose_prior(self, pid, z, info):
        """z = (x, y, theta), information 3x3"""
        z = _f64(z); info = _f64(info); self._check(self.L.gs_add_pose_prior(self.h, int(pid), _d(z), _d(info)))

    def add_pose_xy_prior(self, pid, z, info):
        """position only (the GPS case): z = (x, y), information 2x2"""
        z = _f64(z); info = _f64(info); self._check(self.L.gs_add_pose_xy_prior(self.h, int(pid), _d(z), _d(info)))

    def add_landmark_prior(self, lid, z, info):
        z = _f64(z); info = _f64(info); self._check(self.L.gs_add_landmark_prior(self.h, int(lid), _d(z), _d(info)))

    def add_pose_priors(self, ids, z, info):
        ids = _i32(ids); z = _f64(z); info = _f64(info); self._check(self.L.gs_add_pose_priors(self.h, len(ids), _i(ids), _d(z), _d(info)))

    def add_pose_xy_priors(self, ids, z, info):
        ids = _i32(ids); z = _f64(z); info = _f64(info); self._check(self.L.gs_add_pose_xy_priors(self.h, len(ids), _i(ids), _d(z), _d(info)))

    def add_landmark_priors(self, ids, z, info):
        ids = _i32(ids); z = _f64(z); info = _f64(info); self._check(self.L.gs_add_landmark_priors(self.h, len(ids), _i(ids), _d(z), _d(info)))

    @property
    def n_pose_priors(self): return self._check(self.L.gs_num_pose_priors(self.h))
    @property
    def n_landmark_priors(self): return self._check(self.L.gs_num_landmark_priors(self.h))

    def clear_priors(self):
        self._check(self.L.gs_clear_priors(self.h))

    def prior_chi2(self, kind):
        """e^T Omega e of every prior of the kind ("pose" / "landmark" or 0 / 1) at the current estimates, insertion order"""
        kd = int({"pose": 0, "landmark": 1}.get(kind, kind))
        n = self._check(self.L.gs_get_prior_chi2(self.h, kd, 0, None)); out = np.zeros(n)
        self._check(self.L.gs_get_prior_chi2(self.h, kd, n, _d(out))); return out

    # ---- polar observation edges (gs_add_range_bearing_edge / gs_add_bearing_edge: observation edges with a polar measurement model)
    def add_range_bearing_edge(self, p, l, z, info):
        """z = (range >= 0, bearing in radians), information 2x2 in (range, bearing)"""
        z = _f64(z); info = _f64(info); self._check(self.L.gs_add_range_bearing_edge(self.h, int(p), int(l), _d(z), _d(info)))

    def add_bearing_edge(self, p, l, z, info):
        """bearing only: z in radians, information a scalar >= 0"""
        self._check(self.L.gs_add_bearing_edge(self.h, int(p), int(l), float(z), float(info)))

    def add_range_bearing_edges(self, p, l, z, info):
        p = _i32(p); l = _i32(l); z = _f64(z); info = _f64(info)
        self._check(self.L.gs_add_range_bearing_edges(self.h, len(p), _i(p), _i(l), _d(z), _d(info)))

    def add_bearing_edges(self, p, l, z, info):
        p = _i32(p); l = _i32(l); z = _f64(z); info = _f64(info)
        self._check(self.L.gs_add_bearing_edges(self.h, len(p), _i(p), _i(l), _d(z), _d(info)))

    def num_polar_edges(self):
        return self._check(self.L.gs_num_polar_edges(self.h))

    def polar_edges(self):
        """(observation-edge index, model) of every polar edge, insertion order; model 1 range-bearing, 2 bearing-only"""
        n = self.num_polar_edges(); idx = np.zeros(n, dtype=np.int32); model = np.zeros(n, dtype=np.int32)
        self._check(self.L.gs_get_polar_edges(self.h, n, _i(idx), _i(model))); return idx, model

    # ---- host-only plan (no device work)
    # ---- edge deactivation (gs_set_edge_active ...: per-edge levels; kind "odometry" / "observation", index = insertion index within the kind)
    def set_edge_active(self, kind, index, active=True):
        self._check(self.L.gs_set_edge_active(self.h, int(EDGE_KINDS.get(kind, kind)), int(index), int(bool(active))))

    def set_edges_active(self, kind, indices, active=None):
        """active: one flag per index, or None to switch all the listed edges off"""
        idx = _i32(indices); n = len(idx)
        a = None if active is None else np.ascontiguousarray(np.broadcast_to(np.asarray(active, dtype=bool), (n,)), dtype=np.uint8)
        self._check(self.L.gs_set_edges_active(self.h, int(EDGE_KINDS.get(kind, kind)), n, _i(idx),
                                               None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8))))

    def edges_active(self, kind):
        """bool per edge of the kind, insertion order"""
        kd = int(EDGE_KINDS.get(kind, kind))
        n = self._check(self.L.gs_get_edges_active(self.h, kd, 0, None)); out = np.zeros(n, dtype=np.uint8)
        self._check(self.L.gs_get_edges_active(self.h, kd, n, out.ctypes.data_as(C.POINTER(C.c_uint8)))); return out.astype(bool)

    def activate_all_edges(self):
        self._check(self.L.gs_activate_all_edges(self.h))

    def n_inactive_edges(self, kind):
        return self._check(self.L.gs_num_inactive_edges(self.h, int(EDGE_KINDS.get(kind, kind))))

    def find_isolated_vertex(self):
        """("pose" | "landmark", id) of the first free vertex without a prior and without an active edge, or None"""
        k = C.c_int32(); i = C.c_int32()
        if self._check(self.L.gs_find_isolated_vertex(self.h, C.byref(k), C.byref(i))) == 0:
            return None
        return ("pose", "landmark")[k.value], i.value

    def deactivate_edges_above(self, kind, s_threshold, keep_connected=False):
        """switches off the active edges of the kind with e^T Omega e > s_threshold at the current estimates; returns how many"""
        n = C.c_int32()
        self._check(self.L.gs_deactivate_edges_above(self.h, int(EDGE_KINDS.get(kind, kind)), float(s_threshold), int(bool(keep_connected)), C.byref(n)))
        return n.value

    def plan_build_host(self):
        info = PlanInfo(); self._check(self.L.gs_plan_build_host(self.h, C.byref(info))); return info

    def reserve_device(self, nbytes):
        """takes device memory for the first structure phase now (start-up) instead of inside the first optimize()"""
        self._check(self.L.gs_reserve_device(self.h, int(nbytes)))

    def plan_growths(self):
        """append-only growth steps the current plan has absorbed (0: the plan is a full build)"""
        return self._check(self.L.gs_plan_growths(self.h))

    def growth_refusal(self):
        """why the last structure change was not absorbed by growing the plan ('' if it was)"""
        return self.L.gs_growth_refusal(self.h).decode()

    def plan_export(self):
        n = C.c_int64(0)
        self._check(self.L.gs_plan_export(self.h, None, C.byref(n)))
        out = np.zeros(n.value, dtype=np.int32)
        self._check(self.L.gs_plan_export(self.h, _i(out), C.byref(n)))
        return out

    def debug_schedule(self):
        """the solver launches of the current plan (gs_debug_schedule_export), parsed: the scalar decisions, level lists, the five
        workgroup tables as (n, 2) arrays and the launches of an iteration per mode as (n, 6) arrays
        {kind, first, count, lds, cls, table}"""
        n = C.c_int64(0)
        self._check(self.L.gs_debug_schedule_export(self.h, None, C.byref(n)))
        raw = np.zeros(n.value, dtype=np.int32)
        self._check(self.L.gs_debug_schedule_export(self.h, _i(raw), C.byref(n)))
        names = ("magic", "n_levels", "n_own", "n_shared", "shared_base", "factor_variant", "tables", "leaf_n", "leaf_slot", "leaf_max_f",
                 "n_subtrees", "sub_first", "sub_free", "block_n", "bs_l0", "small_max_npiv", "small_max_f")
        S = {k: int(raw[i]) for i, k in enumerate(names)}
        at = [20]
        def take(cnt, width=1):
            a = raw[at[0]:at[0] + cnt * width].copy(); at[0] += cnt * width
            return a.reshape(cnt, width) if width > 1 else a
        L1 = S["n_levels"] + 1
        S["own_start"] = take(L1); S["shared_start"] = take(L1); S["own_fronts"] = take(S["n_own"]); S["shared_fronts"] = take(S["n_shared"])
        S["tab"] = [take(int(take(1)[0]), 2) for _ in range(5)]
        S["launches_tree"] = take(int(take(1)[0]), 6); S["launches_level"] = take(int(take(1)[0]), 6)
        assert at[0] == len(raw), (at[0], len(raw))
        S["raw"] = raw
        return S

    # ---- front end
    def polar_to_xy(self, az, zen, dist):
        az = _f64(az); zen = _f64(zen); dist = _f64(dist); out = np.zeros((len(az), 2))
        self._check(self.L.gs_polar_to_xy_batch(self.h, len(az), _d(az), _d(zen), _d(dist), _d(out))); return out

    def cone_to_global(self, poses, pose_of_obs, obs):
        poses = _f64(poses, (-1, 3)); obs = _f64(obs, (-1, 4)); po = _i32(pose_of_obs); out = np.zeros((len(obs), 2))
        self._check(self.L.gs_cone_to_global_batch(self.h, len(obs), _d(poses), len(poses), _i(po), _d(obs), _d(out)))
        return out

    def associate(self, poses, pose_of_obs, obs, map_xy, map_type, thr, type_tol=1e-4):
        poses = _f64(poses, (-1, 3)); obs = _f64(obs, (-1, 4)); po = _i32(pose_of_obs)
        map_xy = _f64(map_xy, (-1, 2)); map_type = _i32(map_type); out = np.zeros(len(obs), dtype=np.int32)
        self._check(self.L.gs_associate_batch(self.h, len(obs), _d(poses), len(poses), _i(po), _d(obs), len(map_xy),
                                              _d(map_xy), _i(map_type), float(thr), float(type_tol), _i(out)))
        return out

    # ---- what the call families below share.  A family's C argument list is built in one place: _<family>_resident_args serves the resident
    # call and, through _timed, its time_* twin; _batch_args makes the host inputs of a batch call.  The frame_frontend_* calls keep their
    # prologue inline: a helper there measured 3 to 5 % on a 30 microsecond call.  A numpy array lives as long as the pointer made
    # from it, a parameter struct as long as its byref: the lists keep both.
    def _timed(self, fn, args, reps):
        """a gs_*time_* entry point: the arguments of the call it repeats, then (reps, out_ms); mean milliseconds per call"""
        ms = C.c_double(); self._check(fn(*args, int(reps), C.byref(ms))); return ms.value

    def _batch_args(self, poses, pose_of_obs, obs, map_xy, map_type, map_cov, pose_cov, frame_start=None, typed=True):
        """the host inputs of a batch call, converted and checked: (n, n_frames or None, the C arguments from the handle to the covariances);
        frame_start: the call takes frames; typed=False: it takes no map types"""
        poses = _f64(poses, (-1, 3)); obs = _f64(obs, (-1, 4)); po = _i32(pose_of_obs); map_xy = _f64(map_xy, (-1, 2)); nf = None
        mc = None if map_cov is None else _f64(map_cov, (-1, 4)); pc = None if pose_cov is None else _f64(pose_cov, (-1, 9))
        assert mc is None or len(mc) == len(map_xy); assert pc is None or len(pc) == len(poses)
        a = [self.h, len(obs), _d(poses), len(poses), _i(po), _d(obs)]
        if frame_start is not None:
            fs = _i32(frame_start); nf = len(fs) - 1
            assert len(fs) >= 1
            a += [nf, _i(fs)]
        a += [len(map_xy), _d(map_xy)]
        if typed:
            a.append(_i(_i32(map_type)))
        return len(obs), nf, a + [None if mc is None else _d(mc), None if pc is None else _d(pc)]

    def _resident_head(self, d_poses, n_poses, d_pose_of_obs, d_obs, n, d_pose_cov, params, n_frames=None, d_frame_start=None):
        """what a resident call against the map's covariances begins with: the handle, the observations and their poses, the frames where the
        call takes them, the pose covariances, the gs_nn_params"""
        a = [self.h, int(n), d_poses.ptr, int(n_poses), d_pose_of_obs.ptr, d_obs.ptr]
        if d_frame_start is not None:
            a += [int(n_frames), d_frame_start.ptr]
        return a + [_ptr(d_pose_cov), C.byref(nn_params() if params is None else params)]

    # ---- per-keyframe front end against the resident map
    def _associate_resident_args(self, d_poses, n_poses, d_pose_of_obs, d_obs, n, thr, d_out, type_tol):
        return [self.h, int(n), d_poses.ptr, int(n_poses), d_pose_of_obs.ptr, d_obs.ptr, float(thr), float(type_tol), d_out.ptr]

    def associate_resident(self, d_poses, n_poses, d_pose_of_obs, d_obs, n, thr, d_out, type_tol=1e-4):
        """gs_associate_resident: the resident map (map_append), everything else DeviceArray; asynchronous (synchronize() before reading d_out)."""
        self._check(self.L.gs_associate_resident(*self._associate_resident_args(d_poses, n_poses, d_pose_of_obs, d_obs, n, thr, d_out, type_tol)))

    def time_associate_resident(self, d_poses, n_poses, d_pose_of_obs, d_obs, n, thr, d_out, reps, type_tol=1e-4):
        return self._timed(self.L.gs_debug_time_associate_resident, self._associate_resident_args(d_poses, n_poses, d_pose_of_obs, d_obs, n, thr, d_out, type_tol), reps)

    def map_clear(self): self._check(self.L.gs_map_clear(self.h))
    def map_size(self): return self._check(self.L.gs_map_size(self.h))

    def map_append(self, xy, types):
        xy = _f64(xy, (-1, 2)); ty = _i32(types); self._check(self.L.gs_map_append(self.h, len(ty), _d(xy), _i(ty)))

    def map_set_xy(self, first, xy):
        xy = _f64(xy, (-1, 2)); self._check(self.L.gs_map_set_xy(self.h, int(first), len(xy), _d(xy)))

    def frame_frontend(self, pose, obs, thr, type_tol=1e-4, signed_type=0):
        """(zxy [k,2], gxy [k,2], idx [k]) of one frame's observations [k,4] against the resident map."""
        pose = _f64(pose); obs = _f64(obs, (-1, 4)); k = len(obs)
        z = np.zeros((k, 2)); gx = np.zeros((k, 2)); idx = np.zeros(k, dtype=np.int32)
        self._check(self.L.gs_frame_frontend(self.h, _d(pose), _d(obs), k, float(thr), float(type_tol), int(signed_type), _d(z), _d(gx), _i(idx)))
        return z, gx, idx

    # ---- covariance-gated association (include/graphslam.h): params = NnParams (None: the library's defaults)
    def map_set_cov(self, first, cov):
        cov = _f64(cov, (-1, 4)); self._check(self.L.gs_map_set_cov(self.h, int(first), len(cov), _d(cov)))

    def map_cov(self, first=0, n=None):
        """[n,2,2] covariance blocks of the resident map's cones [first, first + n) (n = None: to the end)"""
        n = self.map_size() - int(first) if n is None else int(n)
        out = np.zeros((max(n, 0), 2, 2)); self._check(self.L.gs_map_get_cov(self.h, int(first), n, _d(out))); return out

    def map_set_cov_from_marginals(self, first, lm_ids):
        ids = _i32(lm_ids); self._check(self.L.gs_map_set_cov_from_marginals(self.h, int(first), len(ids), _i(ids)))

    def associate_nn(self, poses, pose_of_obs, obs, map_xy, map_type, map_cov=None, pose_cov=None, params=None):
        """gs_associate_nn_batch: (index [n] int32, d2 [n], second_d2 [n])"""
        n, _, a = self._batch_args(poses, pose_of_obs, obs, map_xy, map_type, map_cov, pose_cov)
        p = nn_params() if params is None else params
        idx = np.zeros(n, dtype=np.int32); d2 = np.zeros(n); sec = np.zeros(n)
        self._check(self.L.gs_associate_nn_batch(*a, C.byref(p), _i(idx), _d(d2), _d(sec)))
        return idx, d2, sec

    def _associate_nn_resident_args(self, d_poses, n_poses, d_pose_of_obs, d_obs, n, d_out, d_out_d2, d_out_second, d_pose_cov, params):
        return self._resident_head(d_poses, n_poses, d_pose_of_obs, d_obs, n, d_pose_cov, params) + [d_out.ptr, _ptr(d_out_d2), _ptr(d_out_second)]

    def associate_nn_resident(self, d_poses, n_poses, d_pose_of_obs, d_obs, n, d_out, d_out_d2=None, d_out_second=None, d_pose_cov=None, params=None):
        """gs_associate_nn_resident: the resident map and its covariances, everything else DeviceArray; asynchronous (synchronize() before reading)"""
        self._check(self.L.gs_associate_nn_resident(*self._associate_nn_resident_args(d_poses, n_poses, d_pose_of_obs, d_obs, n, d_out, d_out_d2, d_out_second,
                                                                                      d_pose_cov, params)))

    def time_associate_nn_resident(self, d_poses, n_poses, d_pose_of_obs, d_obs, n, d_out, reps, d_out_d2=None, d_out_second=None, d_pose_cov=None, params=None):
        return self._timed(self.L.gs_debug_time_associate_nn_resident,
                           self._associate_nn_resident_args(d_poses, n_poses, d_pose_of_obs, d_obs, n, d_out, d_out_d2, d_out_second, d_pose_cov, params), reps)

    def frame_frontend_nn(self, pose, obs, pose_cov=None, params=None):
        """(zxy [k,2], gxy [k,2], idx [k], d2 [k], second_d2 [k]) of one frame's observations [k,4] against the resident map and its covariances"""
        pose = _f64(pose); obs = _f64(obs, (-1, 4)); k = len(obs); pc = None if pose_cov is None else _f64(pose_cov, (9,))
        p = nn_params() if params is None else params
        z = np.zeros((k, 2)); gx = np.zeros((k, 2)); idx = np.zeros(k, dtype=np.int32); d2 = np.zeros(k); sec = np.zeros(k)
        self._check(self.L.gs_frame_frontend_nn(self.h, _d(pose), None if pc is None else _d(pc), _d(obs), k, C.byref(p), _d(z), _d(gx), _i(idx), _d(d2), _d(sec)))
        return z, gx, idx, d2, sec

    # ---- one-to-one association (include/graphslam.h): frame f is the observations [frame_start[f], frame_start[f + 1])
    def assign_nn(self, poses, pose_of_obs, obs, frame_start, map_xy, map_type, map_cov=None, pose_cov=None, params=None):
        """gs_assign_nn_batch: (index [n] int32, d2 [n])"""
        n, _, a = self._batch_args(poses, pose_of_obs, obs, map_xy, map_type, map_cov, pose_cov, frame_start)
        p = nn_params() if params is None else params
        idx = np.zeros(n, dtype=np.int32); d2 = np.zeros(n)
        self._check(self.L.gs_assign_nn_batch(*a, C.byref(p), _i(idx), _d(d2)))
        return idx, d2

    def _assign_nn_resident_args(self, d_poses, n_poses, d_pose_of_obs, d_obs, n, n_frames, d_frame_start, d_out, d_out_d2, d_pose_cov, params):
        return self._resident_head(d_poses, n_poses, d_pose_of_obs, d_obs, n, d_pose_cov, params, n_frames, d_frame_start) + [d_out.ptr, _ptr(d_out_d2)]

    def assign_nn_resident(self, d_poses, n_poses, d_pose_of_obs, d_obs, n, n_frames, d_frame_start, d_out, d_out_d2=None, d_pose_cov=None, params=None):
        """gs_assign_nn_resident: the resident map and its covariances, everything else DeviceArray; asynchronous (synchronize() before reading)"""
        self._check(self.L.gs_assign_nn_resident(*self._assign_nn_resident_args(d_poses, n_poses, d_pose_of_obs, d_obs, n, n_frames, d_frame_start, d_out, d_out_d2,
                                                                                d_pose_cov, params)))

    def time_assign_nn_resident(self, d_poses, n_poses, d_pose_of_obs, d_obs, n, n_frames, d_frame_start, d_out, reps, d_out_d2=None, d_pose_cov=None, params=None):
        return self._timed(self.L.gs_debug_time_assign_nn_resident,
                           self._assign_nn_resident_args(d_poses, n_poses, d_pose_of_obs, d_obs, n, n_frames, d_frame_start, d_out, d_out_d2, d_pose_cov, params), reps)

    def frame_frontend_assign(self, pose, obs, pose_cov=None, params=None):
        """(zxy [k,2], gxy [k,2], idx [k], d2 [k]) of one frame's observations [k,4], each cone given to at most one of them"""
        pose = _f64(pose); obs = _f64(obs, (-1, 4)); k = len(obs); pc = None if pose_cov is None else _f64(pose_cov, (9,))
        p = nn_params() if params is None else params
        z = np.zeros((k, 2)); gx = np.zeros((k, 2)); idx = np.zeros(k, dtype=np.int32); d2 = np.zeros(k)
        self._check(self.L.gs_frame_frontend_assign(self.h, _d(pose), None if pc is None else _d(pc), _d(obs), k, C.byref(p), _d(z), _d(gx), _i(idx), _d(d2)))
        return z, gx, idx, d2

    # ---- minimum-cost association (include/graphslam.h): the same frames, the matching of largest total gain over each observation's 8 best cones
    def assign_opt(self, poses, pose_of_obs, obs, frame_start, map_xy, map_type, map_cov=None, pose_cov=None, params=None):
        """gs_assign_opt_batch: (index [n] int32, d2 [n], n_admissible [n] int32)"""
        n, _, a = self._batch_args(poses, pose_of_obs, obs, map_xy, map_type, map_cov, pose_cov, frame_start)
        p = nn_params() if params is None else params
        idx = np.zeros(n, dtype=np.int32); d2 = np.zeros(n); na = np.zeros(n, dtype=np.int32)
        self._check(self.L.gs_assign_opt_batch(*a, C.byref(p), _i(idx), _d(d2), _i(na)))
        return idx, d2, na

    def _assign_opt_resident_args(self, d_poses, n_poses, d_pose_of_obs, d_obs, n, n_frames, d_frame_start, d_out, d_out_d2, d_out_na, d_pose_cov, params):
        return (self._resident_head(d_poses, n_poses, d_pose_of_obs, d_obs, n, d_pose_cov, params, n_frames, d_frame_start)
                + [d_out.ptr, _ptr(d_out_d2), _ptr(d_out_na)])

    def assign_opt_resident(self, d_poses, n_poses, d_pose_of_obs, d_obs, n, n_frames, d_frame_start, d_out, d_out_d2=None, d_out_na=None, d_pose_cov=None, params=None):
        """gs_assign_opt_resident: the resident map and its covariances, everything else DeviceArray; asynchronous (synchronize() before reading)"""
        self._check(self.L.gs_assign_opt_resident(*self._assign_opt_resident_args(d_poses, n_poses, d_pose_of_obs, d_obs, n, n_frames, d_frame_start, d_out, d_out_d2,
                                                                                  d_out_na, d_pose_cov, params)))

    def time_assign_opt_resident(self, d_poses, n_poses, d_pose_of_obs, d_obs, n, n_frames, d_frame_start, d_out, reps, d_out_d2=None, d_out_na=None, d_pose_cov=None, params=None):
        return self._timed(self.L.gs_debug_time_assign_opt_resident,
                           self._assign_opt_resident_args(d_poses, n_poses, d_pose_of_obs, d_obs, n, n_frames, d_frame_start, d_out, d_out_d2, d_out_na, d_pose_cov,
                                                          params), reps)

    def frame_frontend_assign_opt(self, pose, obs, pose_cov=None, params=None):
        """(zxy [k,2], gxy [k,2], idx [k], d2 [k], n_admissible [k]) of one frame's observations [k,4], matched at least total d2"""
        pose = _f64(pose); obs = _f64(obs, (-1, 4)); k = len(obs); pc = None if pose_cov is None else _f64(pose_cov, (9,))
        p = nn_params() if params is None else params
        z = np.zeros((k, 2)); gx = np.zeros((k, 2)); idx = np.zeros(k, dtype=np.int32); d2 = np.zeros(k); na = np.zeros(k, dtype=np.int32)
        self._check(self.L.gs_frame_frontend_assign_opt(self.h, _d(pose), None if pc is None else _d(pc), _d(obs), k, C.byref(p), _d(z), _d(gx), _i(idx), _d(d2), _i(na)))
        return z, gx, idx, d2, na

    # ---- joint compatibility (include/graphslam.h): a frame's hypothesis (cone or -1 per observation) gated as a whole and pruned.
    # A frame's record is a dict: joint_d2 [f], n_kept / n_dropped / n_untestable [f] int32, delta [f,3]
    def joint_compat(self, poses, pose_of_obs, obs, frame_start, map_xy, in_index, map_cov=None, pose_cov=None, params=None, jc=None):
        """gs_joint_compat_batch: (index [n] int32, record)"""
        n, nf, a = self._batch_args(poses, pose_of_obs, obs, map_xy, None, map_cov, pose_cov, frame_start, typed=False)
        ii = _i32(in_index)
        assert len(ii) == n
        p = nn_params() if params is None else params; j = jc_params() if jc is None else jc
        idx = np.zeros(n, dtype=np.int32); rec, ra = _jc_record(nf)
        self._check(self.L.gs_joint_compat_batch(*a, C.byref(p), C.byref(j), _i(ii), _i(idx), *ra))
        return idx, rec

    def _joint_compat_resident_args(self, d_poses, n_poses, d_pose_of_obs, d_obs, n, n_frames, d_frame_start, d_in_index, d_out, d_joint_d2, d_n_kept, d_n_dropped,
                                    d_n_untestable, d_delta, d_pose_cov, params, jc):
        return (self._resident_head(d_poses, n_poses, d_pose_of_obs, d_obs, n, d_pose_cov, params, n_frames, d_frame_start)
                + [C.byref(jc_params() if jc is None else jc), d_in_index.ptr, d_out.ptr, _ptr(d_joint_d2), _ptr(d_n_kept), _ptr(d_n_dropped), _ptr(d_n_untestable),
                   _ptr(d_delta)])

    def joint_compat_resident(self, d_poses, n_poses, d_pose_of_obs, d_obs, n, n_frames, d_frame_start, d_in_index, d_out, d_joint_d2=None, d_n_kept=None,
                              d_n_dropped=None, d_n_untestable=None, d_delta=None, d_pose_cov=None, params=None, jc=None):
        """gs_joint_compat_resident: the resident map and its covariances, everything else DeviceArray; asynchronous (synchronize() before reading)"""
        self._check(self.L.gs_joint_compat_resident(*self._joint_compat_resident_args(d_poses, n_poses, d_pose_of_obs, d_obs, n, n_frames, d_frame_start, d_in_index, d_out,
                                                                                      d_joint_d2, d_n_kept, d_n_dropped, d_n_untestable, d_delta, d_pose_cov, params, jc)))

    def time_joint_compat_resident(self, d_poses, n_poses, d_pose_of_obs, d_obs, n, n_frames, d_frame_start, d_in_index, d_out, reps, d_joint_d2=None,
                                   d_n_kept=None, d_n_dropped=None, d_n_untestable=None, d_delta=None, d_pose_cov=None, params=None, jc=None):
        return self._timed(self.L.gs_debug_time_joint_compat_resident,
                           self._joint_compat_resident_args(d_poses, n_poses, d_pose_of_obs, d_obs, n, n_frames, d_frame_start, d_in_index, d_out, d_joint_d2, d_n_kept,
                                                            d_n_dropped, d_n_untestable, d_delta, d_pose_cov, params, jc), reps)

    def frame_frontend_jc(self, pose, obs, pose_cov=None, params=None, jc=None):
        """(zxy [k,2], gxy [k,2], pruned idx [k], the assignment's d2 [k] and n_admissible [k], record of the one frame) — gs_frame_frontend_assign_opt
        followed by the joint test of its result"""
        pose = _f64(pose); obs = _f64(obs, (-1, 4)); k = len(obs); pc = None if pose_cov is None else _f64(pose_cov, (9,))
        p = nn_params() if params is None else params; j = jc_params() if jc is None else jc
        z = np.zeros((k, 2)); gx = np.zeros((k, 2)); idx = np.zeros(k, dtype=np.int32); d2 = np.zeros(k); na = np.zeros(k, dtype=np.int32); rec, ra = _jc_record(1)
        self._check(self.L.gs_frame_frontend_jc(self.h, _d(pose), None if pc is None else _d(pc), _d(obs), k, C.byref(p), C.byref(j), _d(z), _d(gx), _i(idx), _d(d2), _i(na),
                                                *ra))
        return z, gx, idx, d2, na, rec

    # ---- frame localisation (include/graphslam.h): the iterated pose refinement of a frame under its hypothesis.
    # A frame's record is a dict: pose [f,3], cov [f,9], chi2 [f], n_pairs / iterations / status [f] int32
    def localize(self, poses, pose_of_obs, obs, frame_start, map_xy, in_index, map_cov=None, pose_cov=None, params=None, loc=None):
        """gs_localize_batch: the record of every frame"""
        n, nf, a = self._batch_args(poses, pose_of_obs, obs, map_xy, None, map_cov, pose_cov, frame_start, typed=False)
        ii = _i32(in_index)
        assert len(ii) == n
        p = nn_params() if params is None else params; l = loc_params() if loc is None else loc
        rec, ra = _loc_record(nf)
        self._check(self.L.gs_localize_batch(*a, C.byref(p), C.byref(l), _i(ii), *ra))
        return rec

    def _localize_resident_args(self, d_poses, n_poses, d_pose_of_obs, d_obs, n, n_frames, d_frame_start, d_in_index, d_pose, d_cov, d_chi2, d_n_pairs, d_iterations,
                                d_status, d_pose_cov, params, loc):
        return (self._resident_head(d_poses, n_poses, d_pose_of_obs, d_obs, n, d_pose_cov, params, n_frames, d_frame_start)
                + [C.byref(loc_params() if loc is None else loc), d_in_index.ptr, _ptr(d_pose), _ptr(d_cov), _ptr(d_chi2), _ptr(d_n_pairs), _ptr(d_iterations),
                   _ptr(d_status)])

    def localize_resident(self, d_poses, n_poses, d_pose_of_obs, d_obs, n, n_frames, d_frame_start, d_in_index, d_pose=None, d_cov=None, d_chi2=None,
                          d_n_pairs=None, d_iterations=None, d_status=None, d_pose_cov=None, params=None, loc=None):
        """gs_localize_resident: the resident map and its covariances, everything else DeviceArray; asynchronous (synchronize() before reading)"""
        self._check(self.L.gs_localize_resident(*self._localize_resident_args(d_poses, n_poses, d_pose_of_obs, d_obs, n, n_frames, d_frame_start, d_in_index, d_pose, d_cov,
                                                                              d_chi2, d_n_pairs, d_iterations, d_status, d_pose_cov, params, loc)))

    def time_localize_resident(self, d_poses, n_poses, d_pose_of_obs, d_obs, n, n_frames, d_frame_start, d_in_index, reps, d_pose=None, d_cov=None,
                               d_chi2=None, d_n_pairs=None, d_iterations=None, d_status=None, d_pose_cov=None, params=None, loc=None):
        return self._timed(self.L.gs_debug_time_localize_resident,
                           self._localize_resident_args(d_poses, n_poses, d_pose_of_obs, d_obs, n, n_frames, d_frame_start, d_in_index, d_pose, d_cov, d_chi2, d_n_pairs,
                                                        d_iterations, d_status, d_pose_cov, params, loc), reps)

    def debug_localize(self, kernel=-1, d_step=None):
        """gs_debug_localize: force k_localize (0) or k_localize_big (1), -1 by the mean frame size; d_step: a DeviceArray of 3 doubles per frame that
        later localize_resident calls fill with d_f, None to stop"""
        self._check(self.L.gs_debug_localize(self.h, int(kernel), _ptr(d_step)))

    def frame_frontend_localize(self, pose, obs, pose_cov=None, params=None, jc=None, loc=None):
        """frame_frontend_jc's tuple (zxy, gxy, pruned idx, d2, n_admissible, joint record) + the localisation record of the one frame"""
        pose = _f64(pose); obs = _f64(obs, (-1, 4)); k = len(obs); pc = None if pose_cov is None else _f64(pose_cov, (9,))
        p = nn_params() if params is None else params; j = jc_params() if jc is None else jc; l = loc_params() if loc is None else loc
        z = np.zeros((k, 2)); gx = np.zeros((k, 2)); idx = np.zeros(k, dtype=np.int32); d2 = np.zeros(k); na = np.zeros(k, dtype=np.int32)
        (rec, ra), (lr, la) = _jc_record(1), _loc_record(1)
        self._check(self.L.gs_frame_frontend_localize(self.h, _d(pose), None if pc is None else _d(pc), _d(obs), k, C.byref(p), C.byref(j), C.byref(l), _d(z), _d(gx),
                                                      _i(idx), _d(d2), _i(na), *ra, *la))
        return z, gx, idx, d2, na, rec, lr

    # ---- relocalisation (include/graphslam.h): a frame's pose found on the map without a prior.
    # A frame's record is a dict: pose [f,3], count [f], cost [f], seed [f,4], second_count [f], second_pose [f,3], n_seeds [f] int64, status [f]
    def relocalize(self, obs, frame_start, map_xy, map_type, params=None, second=True):
        """gs_relocalize_batch: (record of every frame, index [n], e2 [n]); second=False skips the runner-up's pass (its fields stay zero)"""
        obs = _f64(obs, (-1, 4)); fs = _i32(frame_start); map_xy = _f64(map_xy, (-1, 2)); mt = _i32(map_type); n = len(obs); nf = len(fs) - 1
        assert len(fs) >= 1 and len(mt) == len(map_xy)
        p = reloc_params() if params is None else params
        rec = _reloc_record(nf); ra = _reloc_record_args(rec, second); idx = np.zeros(n, dtype=np.int32); e2 = np.zeros(n)
        self._check(self.L.gs_relocalize_batch(self.h, n, _d(obs), nf, _i(fs), len(map_xy), _d(map_xy), _i(mt), C.byref(p), *ra,
                                               _i(idx), _d(e2)))
        return rec, idx, e2

    def _relocalize_resident_args(self, d_obs, n, n_frames, d_frame_start, d_pose, d_count, d_cost, d_seed, d_second_count, d_second_pose, d_n_seeds, d_status,
                                  d_index, d_e2, params):
        return [self.h, int(n), d_obs.ptr, int(n_frames), d_frame_start.ptr, C.byref(reloc_params() if params is None else params), _ptr(d_pose), _ptr(d_count),
                _ptr(d_cost), _ptr(d_seed), _ptr(d_second_count), _ptr(d_second_pose), _ptr(d_n_seeds), _ptr(d_status), _ptr(d_index), _ptr(d_e2)]

    def relocalize_resident(self, d_obs, n, n_frames, d_frame_start, d_pose=None, d_count=None, d_cost=None, d_seed=None, d_second_count=None,
                            d_second_pose=None, d_n_seeds=None, d_status=None, d_index=None, d_e2=None, params=None):
        """gs_relocalize_resident: the resident map, everything else DeviceArray; asynchronous (synchronize() before reading)"""
        self._check(self.L.gs_relocalize_resident(*self._relocalize_resident_args(d_obs, n, n_frames, d_frame_start, d_pose, d_count, d_cost, d_seed, d_second_count,
                                                                                  d_second_pose, d_n_seeds, d_status, d_index, d_e2, params)))

    def time_relocalize_resident(self, d_obs, n, n_frames, d_frame_start, reps, d_pose=None, d_count=None, d_cost=None, d_seed=None, d_second_count=None,
                                 d_second_pose=None, d_n_seeds=None, d_status=None, d_index=None, d_e2=None, params=None):
        return self._timed(self.L.gs_debug_time_relocalize_resident,
                           self._relocalize_resident_args(d_obs, n, n_frames, d_frame_start, d_pose, d_count, d_cost, d_seed, d_second_count, d_second_pose, d_n_seeds,
                                                          d_status, d_index, d_e2, params), reps)

    def debug_relocalize(self, slice_cones=0):
        """gs_debug_relocalize: the cones p a workgroup of the seed kernel enumerates (0: the launcher's choice); results do not depend on it"""
        self._check(self.L.gs_debug_relocalize(self.h, int(slice_cones)))

    def frame_frontend_relocalize(self, obs, prior_sigma_xy, prior_sigma_theta, reloc=None, params=None, jc=None, loc=None, second=True):
        """(search record, search index, search e2) + frame_frontend_localize's tuple from the found pose under the diagonal prior"""
        obs = _f64(obs, (-1, 4)); k = len(obs)
        r = reloc_params() if reloc is None else reloc
        p = nn_params() if params is None else params; j = jc_params() if jc is None else jc; l = loc_params() if loc is None else loc
        sr = _reloc_record(1); sa = _reloc_record_args(sr, second); si = np.zeros(k, dtype=np.int32); se = np.zeros(k)
        z = np.zeros((k, 2)); gx = np.zeros((k, 2)); idx = np.zeros(k, dtype=np.int32); d2 = np.zeros(k); na = np.zeros(k, dtype=np.int32)
        (rec, ra), (lr, la) = _jc_record(1), _loc_record(1)
        self._check(self.L.gs_frame_frontend_relocalize(self.h, _d(obs), k, C.byref(r), float(prior_sigma_xy), float(prior_sigma_theta), C.byref(p), C.byref(j), C.byref(l),
                                                        *sa, _i(si), _d(se), _d(z), _d(gx), _i(idx), _d(d2), _i(na), *ra, *la))
        return sr, si, se, z, gx, idx, d2, na, rec, lr

    # ---- frame following (include/graphslam.h): pose hypotheses carried from frame to frame on the device.
    # Records are numpy arrays of FOLLOW_STEP [n_steps, n_hyp] and FOLLOW_STATE [n_hyp]; the pruned index is [n_hyp, n]
    @staticmethod
    def _follow_blocks(params, jc, loc, follow):
        return (nn_params() if params is None else params, jc_params() if jc is None else jc, loc_params() if loc is None else loc,
                follow_params() if follow is None else follow)

    def follow(self, poses, obs, frame_start, motion, map_xy, map_type, covs=None, motion_cov=None, map_cov=None, params=None, jc=None, loc=None,
               follow=None, index=True):
        """gs_follow_batch: {"steps", "index" (None with index=False), "state", "best", "n_tracking"} of a run over all frames"""
        poses = _f64(poses, (-1, 3)); obs = _f64(obs, (-1, 4)); fs = _i32(frame_start); map_xy = _f64(map_xy, (-1, 2)); mt = _i32(map_type)
        nh = len(poses); n = len(obs); ns = len(fs) - 1
        mo = None if motion is None else _f64(motion, (-1, 3)); mq = None if motion_cov is None else _f64(motion_cov, (-1, 9))
        cv = None if covs is None else _f64(covs, (-1, 9)); mc = None if map_cov is None else _f64(map_cov, (-1, 4))
        assert len(fs) >= 1 and len(mt) == len(map_xy) and (mo is None or len(mo) >= ns - 1) and (mq is None or len(mq) >= ns - 1)
        assert (cv is None or len(cv) == nh) and (mc is None or len(mc) == len(map_xy))
        p, j, l, f = self._follow_blocks(params, jc, loc, follow)
        steps = np.zeros((max(ns, 0), nh), dtype=FOLLOW_STEP); idx = np.zeros((nh, n), dtype=np.int32) if index else None
        state = np.zeros(nh, dtype=FOLLOW_STATE); best = C.c_int32(-2); nt = C.c_int32(-2)
        o = lambda a: None if a is None else _d(a)
        self._check(self.L.gs_follow_batch(self.h, nh, _d(poses), o(cv), ns, n, _d(obs), _i(fs), o(mo), o(mq), len(map_xy), _d(map_xy), _i(mt), o(mc),
                                           C.byref(p), C.byref(j), C.byref(l), C.byref(f), _vp(steps), None if idx is None else _i(idx),
                                           _vp(state), C.byref(best), C.byref(nt)))
        return {"steps": steps, "index": idx, "state": state, "best": best.value, "n_tracking": nt.value}

    def _follow_resident_args(self, d_poses, n_hyp, d_obs, n, n_steps, d_frame_start, frame_cap, d_motion, d_covs, d_motion_cov, d_steps, d_index, d_state,
                              d_best, params, jc, loc, follow):
        p, j, l, f = self._follow_blocks(params, jc, loc, follow)
        return [self.h, int(n_hyp), _ptr(d_poses), _ptr(d_covs), int(n_steps), int(n), _ptr(d_obs), _ptr(d_frame_start), int(frame_cap), _ptr(d_motion),
                _ptr(d_motion_cov), C.byref(p), C.byref(j), C.byref(l), C.byref(f), _ptr(d_steps), _ptr(d_index), _ptr(d_state), _ptr(d_best)]

    def follow_resident(self, d_poses, n_hyp, d_obs, n, n_steps, d_frame_start, frame_cap, d_motion=None, d_covs=None, d_motion_cov=None, d_steps=None,
                        d_index=None, d_state=None, d_best=None, params=None, jc=None, loc=None, follow=None):
        """gs_follow_resident: the resident map, everything else DeviceArray; asynchronous (synchronize() before reading)"""
        self._check(self.L.gs_follow_resident(*self._follow_resident_args(d_poses, n_hyp, d_obs, n, n_steps, d_frame_start, frame_cap, d_motion, d_covs,
                                                                          d_motion_cov, d_steps, d_index, d_state, d_best, params, jc, loc, follow)))

    def time_follow_resident(self, d_poses, n_hyp, d_obs, n, n_steps, d_frame_start, frame_cap, reps, d_motion=None, d_covs=None, d_motion_cov=None,
                             d_steps=None, d_index=None, d_state=None, d_best=None, params=None, jc=None, loc=None, follow=None):
        """gs_debug_time_follow_resident: mean milliseconds per run, events from the run's first dispatch to its last"""
        return self._timed(self.L.gs_debug_time_follow_resident,
                           self._follow_resident_args(d_poses, n_hyp, d_obs, n, n_steps, d_frame_start, frame_cap, d_motion, d_covs, d_motion_cov, d_steps, d_index,
                                                      d_state, d_best, params, jc, loc, follow), reps)

    def follow_set(self, poses, covs=None):
        """gs_follow_set: put the hypotheses on the handle; the next frame_frontend_follow takes no motion"""
        poses = _f64(poses, (-1, 3)); cv = None if covs is None else _f64(covs, (-1, 9))
        assert cv is None or len(cv) == len(poses)
        self._check(self.L.gs_follow_set(self.h, len(poses), _d(poses), None if cv is None else _d(cv)))
        self._follow_n_hyp = len(poses)

    def follow_get(self):
        """gs_follow_get: (state [n_hyp], best, n_tracking) of the live run"""
        state = np.zeros(FOLLOW_HYP_MAX, dtype=FOLLOW_STATE); nh = C.c_int32(0); best = C.c_int32(-2); nt = C.c_int32(-2)
        self._check(self.L.gs_follow_get(self.h, _vp(state), C.byref(nh), C.byref(best), C.byref(nt)))
        return state[:nh.value].copy(), best.value, nt.value

    def frame_frontend_follow(self, obs, motion=None, motion_cov=None, params=None, jc=None, loc=None, follow=None):
        """gs_frame_frontend_follow: one step of the live run: (steps [n_hyp], index [n_hyp, k], best, n_tracking)"""
        obs = _f64(obs, (-1, 4)); k = len(obs)
        mo = None if motion is None else _f64(motion, (3,)); mq = None if motion_cov is None else _f64(motion_cov, (9,))
        p, j, l, f = self._follow_blocks(params, jc, loc, follow)
        steps = np.zeros(FOLLOW_HYP_MAX, dtype=FOLLOW_STEP); idx = np.zeros(FOLLOW_HYP_MAX * max(k, 1), dtype=np.int32)
        nh = getattr(self, "_follow_n_hyp", 0); best = C.c_int32(-2); nt = C.c_int32(-2)
        self._check(self.L.gs_frame_frontend_follow(self.h, None if mo is None else _d(mo), None if mq is None else _d(mq), _d(obs), k, C.byref(p), C.byref(j),
                                                    C.byref(l), C.byref(f), _vp(steps), _i(idx), C.byref(best), C.byref(nt)))
        return steps[:nh].copy(), idx[:nh * k].reshape(nh, k).copy(), best.value, nt.value

    # ---- cone candidates (include/graphslam.h): unmatched observations tracked into new map cones on the device.
    # Records are numpy arrays of CAND [CAND_MAX] (slot s at [s]) and CAND_STEP [n_steps]
    @staticmethod
    def _cand_blocks(params, cand):
        return nn_params() if params is None else params, cand_params() if cand is None else cand

    @staticmethod
    def _cand_records(table):
        """a table to load: CAND records, slot s at [s] (None: none)"""
        t = np.zeros(0, dtype=CAND) if table is None else np.ascontiguousarray(table, dtype=CAND).reshape(-1)
        return t, (_vp(t) if len(t) else None)

    def cand(self, poses, obs, frame_start, in_idx=None, pose_covs=None, table=None, params=None, cand=None):
        """gs_cand_batch: {"steps", "cand_id", "cand_slot", "table", "n_live"} of a run over all frames from the table given (None: empty)"""
        poses = _f64(poses, (-1, 3)); obs = _f64(obs, (-1, 4)); fs = _i32(frame_start); n = len(obs); ns = len(fs) - 1
        pc = None if pose_covs is None else _f64(pose_covs, (-1, 9)); ii = None if in_idx is None else _i32(in_idx)
        assert len(fs) >= 1 and len(poses) >= ns and (pc is None or len(pc) >= ns) and (ii is None or len(ii) == n)
        p, c = self._cand_blocks(params, cand); tab, tp = self._cand_records(table)
        steps = np.zeros(max(ns, 0), dtype=CAND_STEP); cid = np.zeros(n, dtype=np.int32); slot = np.zeros(n, dtype=np.int32)
        out = np.zeros(CAND_MAX, dtype=CAND); nl = C.c_int32(-2)
        self._check(self.L.gs_cand_batch(self.h, ns, n, _d(obs), _i(fs), _d(poses), None if pc is None else _d(pc), None if ii is None else _i(ii), len(tab), tp,
                                         C.byref(p), C.byref(c), _vp(steps), _i(cid), _i(slot), _vp(out), C.byref(nl)))
        return {"steps": steps, "cand_id": cid, "cand_slot": slot, "table": out, "n_live": nl.value}

    def _cand_resident_args(self, d_obs, n, n_steps, d_frame_start, frame_cap, d_poses, d_pose_covs, d_in_idx, n_in, d_table, d_steps, d_cand_id, d_cand_slot,
                            d_out_table, d_meta, params, cand):
        p, c = self._cand_blocks(params, cand)
        return [self.h, int(n_steps), int(n), _ptr(d_obs), _ptr(d_frame_start), int(frame_cap), _ptr(d_poses), _ptr(d_pose_covs), _ptr(d_in_idx), int(n_in),
                _ptr(d_table), C.byref(p), C.byref(c), _ptr(d_steps), _ptr(d_cand_id), _ptr(d_cand_slot), _ptr(d_out_table), _ptr(d_meta)]

    def cand_resident(self, d_obs, n, n_steps, d_frame_start, frame_cap, d_poses, d_pose_covs=None, d_in_idx=None, n_in=0, d_table=None, d_steps=None,
                      d_cand_id=None, d_cand_slot=None, d_out_table=None, d_meta=None, params=None, cand=None):
        """gs_cand_resident: everything DeviceArray; asynchronous (synchronize() before reading)"""
        self._check(self.L.gs_cand_resident(*self._cand_resident_args(d_obs, n, n_steps, d_frame_start, frame_cap, d_poses, d_pose_covs, d_in_idx, n_in, d_table,
                                                                      d_steps, d_cand_id, d_cand_slot, d_out_table, d_meta, params, cand)))

    def time_cand_resident(self, d_obs, n, n_steps, d_frame_start, frame_cap, d_poses, reps, d_pose_covs=None, d_in_idx=None, n_in=0, d_table=None, d_steps=None,
                           d_cand_id=None, d_cand_slot=None, d_out_table=None, d_meta=None, params=None, cand=None):
        """gs_debug_time_cand_resident: mean milliseconds per run, events from the run's first dispatch to its last"""
        return self._timed(self.L.gs_debug_time_cand_resident,
                           self._cand_resident_args(d_obs, n, n_steps, d_frame_start, frame_cap, d_poses, d_pose_covs, d_in_idx, n_in, d_table, d_steps, d_cand_id,
                                                    d_cand_slot, d_out_table, d_meta, params, cand), reps)

    def cand_clear(self):
        self._check(self.L.gs_cand_clear(self.h))

    def cand_set(self, table):
        """gs_cand_set: load CAND records into the live table, slot s from [s]"""
        tab, tp = self._cand_records(table)
        self._check(self.L.gs_cand_set(self.h, len(tab), tp))

    def cand_get(self):
        """gs_cand_get: (table [CAND_MAX], next_id, step, n_live) of the live table"""
        out = np.zeros(CAND_MAX, dtype=CAND); ni = C.c_int32(-2); t = C.c_int32(-2); nl = C.c_int32(-2)
        self._check(self.L.gs_cand_get(self.h, _vp(out), C.byref(ni), C.byref(t), C.byref(nl)))
        return out, ni.value, t.value, nl.value

    def cand_take_confirmed(self):
        """gs_cand_take_confirmed: the confirmed records in ascending id; their slots are free afterwards"""
        out = np.zeros(CAND_MAX, dtype=CAND); n = C.c_int32(0)
        self._check(self.L.gs_cand_take_confirmed(self.h, CAND_MAX, _vp(out), C.byref(n)))
        return out[:n.value].copy()

    def cand_promote(self):
        """the confirmed candidates taken out of the table and appended to the resident map with their covariances (gs_map_append,
        gs_map_set_cov); returns (records, the map index of the first) — adding the landmarks to the graph stays with the caller"""
        rec = self.cand_take_confirmed(); first = self.map_size()
        if len(rec):
            self.map_append(rec["xy"], rec["type"]); self.map_set_cov(first, rec["cov"])
        return rec, first

    def frame_frontend_candidates(self, pose, obs, in_idx=None, pose_cov=None, params=None, cand=None):
        """gs_frame_frontend_candidates: one step on the live table: (step record, cand_id [k], cand_slot [k])"""
        pose = _f64(pose, (3,)); obs = _f64(obs, (-1, 4)); k = len(obs)
        pc = None if pose_cov is None else _f64(pose_cov, (9,)); ii = None if in_idx is None else _i32(in_idx)
        assert ii is None or len(ii) == k
        p, c = self._cand_blocks(params, cand)
        step = np.zeros(1, dtype=CAND_STEP); cid = np.zeros(max(k, 1), dtype=np.int32); slot = np.zeros(max(k, 1), dtype=np.int32)
        self._check(self.L.gs_frame_frontend_candidates(self.h, _d(pose), None if pc is None else _d(pc), _d(obs), k, None if ii is None else _i(ii), C.byref(p),
                                                        C.byref(c), _vp(step), _i(cid), _i(slot)))
        return step[0].copy(), cid[:k].copy(), slot[:k].copy()

    # ---- map twins (include/graphslam.h): duplicate cones found, fused and merged in the graph.  params = DupParams (None: the defaults)
    @staticmethod
    def _host_map(map_xy, map_type, map_cov):
        """a host map, converted and checked: (n, the C arguments n, xy, type, covariances or NULL)"""
        xy = _f64(map_xy, (-1, 2)); ty = _i32(map_type); n = len(ty); mc = None if map_cov is None else _f64(map_cov, (-1, 4))
        assert len(xy) == n and (mc is None or len(mc) == n)
        return n, [n, _d(xy), _i(ty), None if mc is None else _d(mc)]

    def map_twins(self, map_xy, map_type, map_cov=None, params=None):
        """gs_map_twins_batch: (twin [n] int32, d2 [n], second_d2 [n], n_admissible [n] int32) of a host map"""
        n, a = self._host_map(map_xy, map_type, map_cov)
        p = dup_params() if params is None else params
        tw = np.zeros(max(n, 1), dtype=np.int32); d2 = np.zeros(max(n, 1)); sec = np.zeros(max(n, 1)); na = np.zeros(max(n, 1), dtype=np.int32)
        self._check(self.L.gs_map_twins_batch(self.h, *a, C.byref(p), _i(tw), _d(d2), _d(sec), _i(na)))
        return tw[:n].copy(), d2[:n].copy(), sec[:n].copy(), na[:n].copy()

    def _map_twins_resident_args(self, d_twin, d_d2, d_second, d_n_admissible, params):
        return [self.h, C.byref(dup_params() if params is None else params), _ptr(d_twin), _ptr(d_d2), _ptr(d_second), _ptr(d_n_admissible)]

    def map_twins_resident(self, d_twin, d_d2=None, d_second=None, d_n_admissible=None, params=None):
        """gs_map_twins_resident: the resident map and its covariances, outputs DeviceArray; asynchronous (synchronize() before reading)"""
        self._check(self.L.gs_map_twins_resident(*self._map_twins_resident_args(d_twin, d_d2, d_second, d_n_admissible, params)))

    def time_map_twins_resident(self, d_twin, reps, d_d2=None, d_second=None, d_n_admissible=None, params=None):
        """gs_debug_time_map_twins_resident: mean milliseconds per call, events on the search's dispatch"""
        return self._timed(self.L.gs_debug_time_map_twins_resident, self._map_twins_resident_args(d_twin, d_d2, d_second, d_n_admissible, params), reps)

    def time_map_merge_twins(self, reps, params=None):
        """gs_debug_time_map_merge_twins: mean milliseconds of the consolidation's four dispatches over the resident map, which stays as it is"""
        return self._timed(self.L.gs_debug_time_map_merge_twins, [self.h, C.byref(dup_params() if params is None else params)], reps)

    def map_merge_twins_batch(self, map_xy, map_type, map_cov=None, params=None):
        """gs_map_merge_twins_batch: (xy [n_out,2], type [n_out], cov [n_out,2,2] or None, remap [n], info) of a host map"""
        n, a = self._host_map(map_xy, map_type, map_cov)
        p = dup_params() if params is None else params
        m = max(n, 1)
        oxy = np.zeros((m, 2)); oty = np.zeros(m, dtype=np.int32); ocv = None if map_cov is None else np.zeros((m, 2, 2)); rm = np.zeros(m, dtype=np.int32)
        info = np.zeros(1, dtype=DUP_INFO)
        self._check(self.L.gs_map_merge_twins_batch(self.h, *a, C.byref(p), _d(oxy), _i(oty), None if ocv is None else _d(ocv), _i(rm), _vp(info)))
        k = int(info[0]["n_out"])
        return oxy[:k].copy(), oty[:k].copy(), None if ocv is None else ocv[:k].copy(), rm[:n].copy(), info[0].copy()

    def map_merge_twins(self, params=None):
        """gs_map_merge_twins: the resident map consolidated in place; (remap [map size before], info)"""
        p = dup_params() if params is None else params
        n = self.map_size(); rm = np.zeros(max(n, 1), dtype=np.int32); info = np.zeros(1, dtype=DUP_INFO)
        self._check(self.L.gs_map_merge_twins(self.h, C.byref(p), len(rm), _i(rm), _vp(info)))
        return rm[:n].copy(), info[0].copy()

    def map_xy(self, first=0, n=None):
        """gs_map_get_xy: (xy [n,2], type [n]) of the resident map's cones [first, first + n) (n = None: to the end)"""
        n = self.map_size() - int(first) if n is None else int(n)
        xy = np.zeros((max(n, 1), 2)); ty = np.zeros(max(n, 1), dtype=np.int32)
        self._check(self.L.gs_map_get_xy(self.h, int(first), n, _d(xy), _i(ty)))
        return xy[:max(n, 0)].copy(), ty[:max(n, 0)].copy()

    def merge_landmarks(self, keep_id, drop_id):
        """gs_merge_landmarks: drop's observation edges and priors re-attached to keep, drop erased"""
        self._check(self.L.gs_merge_landmarks(self.h, int(keep_id), int(drop_id)))

    def map_consolidate(self, lm_ids, params=None):
        """The resident map consolidated (gs_map_merge_twins) and the graph with it: lm_ids[j] is the graph id of map cone j (-1: not in the
        graph).  For every twin pair whose two cones are in the graph the dropped cone's landmark is merged into the keeper's
        (gs_merge_landmarks) and the keeper's estimate set to the fused position.  Returns (remap, new_lm_ids, info): new_lm_ids[k] is the graph
        id of cone k of the consolidated map — of a pair the keeper's, or the dropped cone's where only that one was in the graph."""
        ids = _i32(lm_ids); n = self.map_size()
        assert len(ids) == n
        remap, info = self.map_merge_twins(params)
        new_ids = np.full(int(info["n_out"]), -1, dtype=np.int32)
        xy, _ = self.map_xy()
        seen = {}
        for old in range(n):
            k = int(remap[old])
            if k not in seen:
                seen[k] = old; new_ids[k] = ids[old]
                continue
            a, b = seen[k], old                             # a twin pair: a < b, a the keeper
            if ids[a] >= 0 and ids[b] >= 0:
                self.merge_landmarks(int(ids[a]), int(ids[b])); self.set_landmark_estimate(int(ids[a]), xy[k])
            elif ids[b] >= 0:
                new_ids[k] = ids[b]
        return remap, new_ids, info

    # ---- pose-window shards (one handle per rank / GPU)
    def dist_configure(self, rank, world):
        self._check(self.L.gs_dist_configure(self.h, int(rank), int(world)))

    # rank-local ingestion (include/graphslam.h, gs_dist_set_landmark_windows)
    def dist_window_starts(self, world):
        out = np.zeros(world + 1, dtype=np.int32)
        self._check(self.L.gs_dist_window_starts(self.h, out.ctypes.data_as(C.POINTER(C.c_int32)), len(out)))
        return out

    def dist_local_landmark_windows(self, n_landmarks):
        a = np.zeros(n_landmarks, dtype=np.uint64); b = np.zeros(n_landmarks, dtype=np.uint64); u = C.POINTER(C.c_uint64)
        self._check(self.L.gs_dist_local_landmark_windows(self.h, a.ctypes.data_as(u), b.ctypes.data_as(u), n_landmarks))
        return a, b

    def dist_share_landmark_windows(self):
        self._check(self.L.gs_dist_share_landmark_windows(self.h))

    def dist_set_landmark_windows(self, seen_interior, seen_first):
        a = np.ascontiguousarray(seen_interior, dtype=np.uint64); b = np.ascontiguousarray(seen_first, dtype=np.uint64); u = C.POINTER(C.c_uint64)
        assert len(a) == len(b)
        self._check(self.L.gs_dist_set_landmark_windows(self.h, a.ctypes.data_as(u), b.ctypes.data_as(u), len(a)))

    def load_bench_graph_shard(self, g, rank, world, masks=None):
        """Rank-local ingestion of the arrays bench_graph makes: every vertex and odometry edge, the observation edges of this rank's window, of the
        windows' first poses and of the fixed poses only, and the whole-graph landmark windows (`masks`, default: landmark_windows(g, world)).
        Returns the boolean selection of g's observation edges that went in (the handle's edge k is g's edge flatnonzero(keep)[k])."""
        N, M = len(g["pose_est"]), len(g["lm_est"])
        self.add_poses(np.arange(N), g["pose_est"]); self.add_landmarks(np.arange(M), g["lm_est"])
        self.add_odometry_edges(g["pp_i"], g["pp_j"], g["pp_z"], g["pp_info"])
        fixed = np.zeros(N, dtype=bool)
        for i in g["fixed_poses"]:
            self.set_fixed_pose(int(i)); fixed[int(i)] = True
        for l in g["fixed_landmarks"]:
            self.set_fixed_landmark(int(l))
        self.dist_configure(rank, world)
        first = self.dist_window_starts(world)
        p = np.asarray(g["pl_p"])
        keep = ((p >= first[rank]) & (p < first[rank + 1])) | np.isin(p, first[1:world]) | fixed[p]
        self.add_observation_edges(p[keep], np.asarray(g["pl_l"])[keep], np.asarray(g["pl_z"])[keep], np.asarray(g["pl_info"])[keep])
        if masks is None:
            masks = landmark_windows(g, world)
        self.dist_set_landmark_windows(*masks)
        return keep

    def dist_exchange_doubles(self):
        return int(self.L.gs_dist_exchange_doubles(self.h))

    def dist_set_exchange_buffer(self, device_ptr):
        self._check(self.L.gs_dist_set_exchange_buffer(self.h, C.c_void_p(device_ptr)))

    def dist_comm_init(self, unique_id, rank, world):
        """ncclCommInitRank inside the library (collective: every rank calls it with the id rank 0 made, dist_unique_id())."""
        self._check(self.L.gs_dist_comm_init(self.h, bytes(unique_id), int(rank), int(world)))

    def dist_set_communicator(self, comm_ptr):
        self._check(self.L.gs_dist_set_communicator(self.h, C.c_void_p(comm_ptr)))

    def dist_iterate(self):
        """one sharded iteration, all from C++: local half -> ncclAllReduce of the exchange buffer -> finish"""
        return self._check(self.L.gs_dist_iterate(self.h))

    def dist_optimize(self, iterations=10):
        st = Stats(); st.struct_size = C.sizeof(Stats)
        done = self._check(self.L.gs_dist_optimize(self.h, int(iterations), C.byref(st)))
        return done, st

    def time_exchange(self, reps):
        return self._timed(self.L.gs_debug_time_exchange, [self.h], reps)

    def dist_iterate_local(self):
        self._check(self.L.gs_dist_iterate_local(self.h))

    def dist_iterate_finish(self):
        self._check(self.L.gs_dist_iterate_finish(self.h))

    def dist_read_exchange(self):
        out = np.zeros(max(self.dist_exchange_doubles(), 1))
        self._check(self.L.gs_dist_read_exchange(self.h, _d(out)))
        return out[:self.dist_exchange_doubles()]

    def dist_write_exchange(self, buf):
        buf = _f64(buf)
        if len(buf) == 0:
            buf = np.zeros(1)
        self._check(self.L.gs_dist_write_exchange(self.h, _d(buf)))

    def dist_known(self):
        """(pose_known, lm_known, pose_primary, lm_primary) boolean arrays, insertion order."""
        N, M = self.n_poses, self.n_landmarks
        a = [np.zeros(max(N, 1), dtype=np.uint8), np.zeros(max(M, 1), dtype=np.uint8),
             np.zeros(max(N, 1), dtype=np.uint8), np.zeros(max(M, 1), dtype=np.uint8)]
        u8 = C.POINTER(C.c_uint8)
        self._check(self.L.gs_dist_known(self.h, *[x.ctypes.data_as(u8) for x in a]))
        return a[0][:N].astype(bool), a[1][:M].astype(bool), a[2][:N].astype(bool), a[3][:M].astype(bool)

    # ---- convenience: load the arrays of track.bench_graph (ids = indices)
    def load_bench_graph(self, g):
        N, M = len(g["pose_est"]), len(g["lm_est"])
        self.add_poses(np.arange(N), g["pose_est"]); self.add_landmarks(np.arange(M), g["lm_est"])
        self.add_odometry_edges(g["pp_i"], g["pp_j"], g["pp_z"], g["pp_info"])
        self.add_observation_edges(g["pl_p"], g["pl_l"], g["pl_z"], g["pl_info"])
        for i in g["fixed_poses"]:
            self.set_fixed_pose(int(i))
        for l in g["fixed_landmarks"]:
            self.set_fixed_landmark(int(l))


def landmark_windows(g, world):
    """The whole-graph landmark windows of gs_dist_set_landmark_windows, from bench_graph arrays in numpy: (seen_interior, seen_first), uint64 per landmark,
    bit w = an interior pose / the first pose of window w observes it (windows = contiguous runs of the FREE poses, ceil(w * n_free / world) first)."""
    N, M = len(g["pose_est"]), len(g["lm_est"])
    fixed_p = np.zeros(N, dtype=bool); fixed_p[np.asarray(g["fixed_poses"], dtype=np.int64)] = True
    fixed_l = np.zeros(M, dtype=bool); fixed_l[np.asarray(g["fixed_landmarks"], dtype=np.int64)] = True
    fp = np.cumsum(~fixed_p) - 1; nfree = int((~fixed_p).sum())
    wf = np.array([(w * nfree + world - 1) // world for w in range(world + 1)], dtype=np.int64)
    p = np.asarray(g["pl_p"]); l = np.asarray(g["pl_l"]); ok = ~fixed_p[p] & ~fixed_l[l]
    fpe = fp[p[ok]]; le = l[ok]
    w = np.minimum(np.searchsorted(wf, fpe, side="right") - 1, world - 1)
    first = (w >= 1) & (fpe == wf[w])
    seen_interior = np.zeros(M, dtype=np.uint64); seen_first = np.zeros(M, dtype=np.uint64)
    for x in range(world):
        sel = w == x
        seen_interior[np.unique(le[sel & ~first])] |= np.uint64(1 << x)
        seen_first[np.unique(le[sel & first])] |= np.uint64(1 << x)
    return seen_interior, seen_first


class Slam:
    """Mirror of the graph side of class Slam (reference src/slam.cpp:298-338 performSLAM and what it calls)."""

    def __init__(self, cfg=None, _handle=None, debug=None, **kw):
        self.L = lib()
        self._owned = _handle is None
        if _handle is not None:
            self.h = C.c_void_p(_handle)
        else:
            if cfg is None:
                cfg = default_config(**kw)
            h = C.c_void_p()
            rc = self.L.gs_slam_create(C.byref(cfg), C.byref(h))
            if rc < 0:
                raise GsError(rc, (self.L.gs_last_error() or b"").decode())
            self.h = h
        self.graph = Graph(_handle=self.L.gs_slam_graph(self.h))
        if _handle is None and (DEFAULT_DEBUG or debug):
            self.graph.set_debug(**dict(DEFAULT_DEBUG, **(debug or {})))

    def _check(self, rc):
        if rc < 0:
            raise GsError(rc, (self.L.gs_last_error() or b"").decode())
        return rc

    def close(self):
        if getattr(self, "h", None) and self._owned:
            self.L.gs_slam_destroy(self.h)
        self.h = None
        if getattr(self, "graph", None) is not None:
            self.graph.h = None                    # borrowed from the slam handle: gone with it (a NULL handle is refused by the C-ABI)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def perform_slam(self, pose, cones_4xk):
        """cones: [K,4] rows (az deg, zen deg, dist m, type) = columns of the reference's collector matrix."""
        pose = _f64(pose); cones = _f64(cones_4xk, (-1, 4))
        self._check(self.L.gs_slam_perform(self.h, _d(pose), _d(cones), len(cones)))

    @property
    def map_size(self): return self._check(self.L.gs_slam_map_size(self.h))
    @property
    def loop_closed(self): return bool(self._check(self.L.gs_slam_loop_closed(self.h)))
    @property
    def current_cone_index(self): return self._check(self.L.gs_slam_current_cone_index(self.h))

    def map(self):
        n = self.map_size; xy = np.zeros((n, 2)); ty = np.zeros(n, dtype=np.int32)
        self._check(self.L.gs_slam_get_map(self.h, n, _d(xy), _i(ty))); return xy, ty

    def map_covariances(self):
        """[n,2,2] covariance of every map cone, map order (computes the marginals of the mirror's graph)"""
        n = self.map_size; out = np.zeros((n, 2, 2))
        self._check(self.L.gs_slam_get_map_covariances(self.h, n, _d(out))); return out

    def send_pose(self):
        o = np.zeros(3); self._check(self.L.gs_slam_get_send_pose(self.h, _d(o))); return o

    # ---- frame collector and output encoders (reference Slam::nextCone / initializeCollection / sendCones)
    def collect_direction(self, object_id, azimuth_deg, zenith_deg):
        return self._check(self.L.gs_slam_collect_direction(self.h, int(object_id), float(azimuth_deg), float(zenith_deg)))

    def collect_distance(self, object_id, distance):
        return self._check(self.L.gs_slam_collect_distance(self.h, int(object_id), float(distance)))

    def collect_type(self, object_id, cone_type):
        return self._check(self.L.gs_slam_collect_type(self.h, int(object_id), int(cone_type)))

    def collect_flush(self, pose):
        """Extracts the collected frame ([K,4] rows az, zen, dist, type), resets the collector, runs perform_slam on it."""
        pose = _f64(pose); k = C.c_int32(0); buf = np.zeros((1000, 4))
        self._check(self.L.gs_slam_collect_flush(self.h, _d(pose), C.byref(k), _d(buf)))
        return buf[:k.value].copy()

    # ---- odometry intake and pose output (reference Slam::nextSplitPose / nextPose / nextYawRate / sendPose)
    def set_gps_reference(self, lat, lon): self._check(self.L.gs_slam_set_gps_reference(self.h, float(lat), float(lon)))
    def next_wgs84(self, lat, lon): self._check(self.L.gs_slam_next_wgs84(self.h, float(lat), float(lon)))
    def next_heading(self, north_heading): self._check(self.L.gs_slam_next_heading(self.h, float(north_heading)))
    def next_geolocation(self, lat, lon, heading): self._check(self.L.gs_slam_next_geolocation(self.h, float(lat), float(lon), float(heading)))
    def next_yaw_rate(self, wz): self._check(self.L.gs_slam_next_yaw_rate(self.h, float(wz)))

    def set_sample_times(self, yaw_received_us, last_cone_us):
        self._check(self.L.gs_slam_set_sample_times(self.h, int(yaw_received_us), int(last_cone_us)))

    def odometry(self):
        o = np.zeros(4); self._check(self.L.gs_slam_get_odometry(self.h, _d(o))); return o

    def encode_pose(self):
        o = np.zeros(3, dtype=np.float32); self._check(self.L.gs_slam_encode_pose(self.h, o.ctypes.data_as(C.POINTER(C.c_float)))); return o

    def encode_cones(self, cones_per_packet):
        n = int(cones_per_packet); az = np.zeros(n, dtype=np.float32); di = np.zeros(n, dtype=np.float32); ty = np.zeros(n, dtype=np.int32)
        self._check(self.L.gs_slam_encode_cones(self.h, n, az.ctypes.data_as(C.POINTER(C.c_float)), di.ctypes.data_as(C.POINTER(C.c_float)), _i(ty)))
        return az, di, ty


def cone_encode(cone_xy, pose, reference_quirks=0):
    """Product implementation of Cone::getDirection / getDistance (reference src/cone.cpp:34-53): (azimuth deg, distance) as float32."""
    L = lib(); az, di = C.c_float(), C.c_float(); c = _f64(cone_xy); p = _f64(pose)
    rc = L.gs_cone_encode(_d(c), _d(p), int(reference_quirks), C.byref(az), C.byref(di))
    if rc != 0: raise GsError(rc, (L.gs_last_error() or b"").decode())
    return np.float32(az.value), np.float32(di.value)


def wgs84_to_cartesian(ref_latlon, pos_latlon):
    """Product implementation of the reference's wgs84::toCartesian (host side, no device needed)."""
    L = lib(); o = np.zeros(2); r = _f64(ref_latlon); p = _f64(pos_latlon)
    if L.gs_wgs84_to_cartesian(_d(r), _d(p), _d(o)) != 0: raise GsError("gs_wgs84_to_cartesian failed")
    return o


def wgs84_from_cartesian(ref_latlon, xy):
    L = lib(); o = np.zeros(2); r = _f64(ref_latlon); p = _f64(xy)
    if L.gs_wgs84_from_cartesian(_d(r), _d(p), _d(o)) != 0: raise GsError("gs_wgs84_from_cartesian failed")
    return o



class Shell:
    """The microservice shell (reference src/opendlv-logic-cfsd18-sensation-slam.cpp:49-119), decoded-message boundary."""
    WGS84, ANGULAR_VELOCITY, HEADING, GEOLOCATION, OBJECT_TYPE, OBJECT_DIRECTION, OBJECT_DISTANCE = 19, 1031, 1051, 1116, 1131, 1133, 1134

    def __init__(self, argv, device=-1):
        self.L = lib()
        arr = (C.c_char_p * len(argv))(*[a.encode() for a in argv])
        h = C.c_void_p()
        rc = self.L.gs_shell_create(len(argv), arr, int(device), C.byref(h))
        if rc < 0:
            raise GsError(rc, (self.L.gs_last_error() or b"").decode())
        self.h = h
        self.slam = Slam(_handle=self.L.gs_shell_slam(self.h))

    def _check(self, rc):
        if rc < 0:
            raise GsError(rc, (self.L.gs_last_error() or b"").decode())
        return rc

    def close(self):
        if getattr(self, "h", None):
            self.L.gs_shell_destroy(self.h)
            self.slam.h = None                     # the shell owned it: the borrowed handles must not outlive it
            self.slam.graph.h = None
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def on_message(self, data_type, sender_stamp, sample_time_us, now_us, object_id=0, v=(0.0, 0.0, 0.0)):
        m = ShellMsg(); m.data_type = int(data_type); m.sender_stamp = int(sender_stamp); m.sample_time_us = int(sample_time_us)
        m.object_id = int(object_id)
        for i, x in enumerate(v):
            m.v[i] = float(x)
        return self._check(self.L.gs_shell_on_message(self.h, C.byref(m), int(now_us)))

    def poll(self, now_us):
        return self._check(self.L.gs_shell_poll(self.h, int(now_us)))

    def take_output(self):
        n = self._check(self.L.gs_shell_pending_output(self.h))
        buf = (ShellMsg * max(n, 1))()
        n = self._check(self.L.gs_shell_take_output(self.h, n, buf))
        return [(m.data_type, m.sender_stamp, m.sample_time_us, m.object_id, (m.v[0], m.v[1], m.v[2])) for m in buf[:n]]

    def counters(self):
        a = (C.c_int64 * 2)(); self._check(self.L.gs_shell_counters(self.h, a)); return int(a[0]), int(a[1])

    @property
    def cid(self): return self._check(self.L.gs_shell_cid(self.h))
