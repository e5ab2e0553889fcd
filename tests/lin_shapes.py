"""The smallest graphs that reach each path of the fused linearisation kernel (TEST-ONLY; deterministic).

k_linearize_ell<T> gives a pose T lanes and each lane R = ceil(kmax / T) observation slots (kmax: the most observations of one pose); a wave
tile is 64 / T consecutive poses.  The planner picks T = 8 for every graph below ~24 000 poses, so the cases here force T
(gs_debug_options.ell_lanes) and set the observations per pose to reach the R they name.  Every graph has
  * anisotropic information matrices, a few of them weak (1e-3 of the others);
  * a fixed first pose that has observations, one fixed landmark that a free pose sees too, and the edge between the two fixed ones;
  * one pose with no observation; one duplicated pose-landmark edge (except where kmax = 1 leaves no room for it);
  * extra odometry edges so that one pose (the hub) has max(5, T + 1) incidences — more than T, so the loop over q0 + h + T runs;
  * one landmark seen from a pose of each of the first three wave tiles (at T = 1 seventy poses are two tiles: from both);
  * a last wave tile that is not full.
CASES maps a name to its recipe and to what the census (test_lin_exact_cpu.py) must find in the plan."""
import numpy as np

import robust_ref as rr

LIN_R = 4                      # observation slots per lane of the fused kernel (gs::LIN_R); more: the gather kernels
FAR = (4e4, -3e4)


def _spd2(rng, scale):
    phi = rng.uniform(0, np.pi); c, s = np.cos(phi), np.sin(phi); R = np.array([[c, -s], [s, c]])
    S = R @ np.diag([rng.uniform(20, 200), rng.uniform(0.5, 5)]) @ R.T * scale
    return ((S + S.T) / 2).reshape(4)


def _spd3(rng, scale):
    A = rng.normal(size=(3, 3)); S = (A @ np.diag([300.0, 20.0, 900.0]) @ A.T + np.diag([5.0, 5.0, 50.0])) * scale
    return ((S + S.T) / 2).reshape(9)


def counts_for(N, kmax, T, full):
    """observations per pose: `full`: kmax everywhere; else 0 .. kmax in a cycle (kmax <= 5) or mostly 0 .. 4 with every 7th pose near kmax
    (every slot of every lane gets edges at some pose, the graph stays small)"""
    if full:
        c = np.full(N, kmax)
    elif kmax <= 5:
        c = np.arange(N) % (kmax + 1)
    else:
        high = [kmax, kmax - 1, kmax - T, kmax - T + 1, (kmax + 1) // 2, kmax - 2 * T + 1]
        c = np.arange(N) % 5
        for t, p in enumerate(range(4, N, 7)):
            c[p] = max(high[t % len(high)], 1)
    c = c.copy(); c[0] = max(c[0], 1); c[min(3, N - 1)] = 0
    if kmax >= 2:
        c[2] = max(c[2], 2)
    if c.max() < kmax:
        c[min(4, N - 1)] = kmax
    return c


def make(N=70, kmax=4, T=1, n_lms=None, full=False, stride=7, seed=0, far=False, robust=False):
    rng = np.random.default_rng(1000 + seed)
    M = int(n_lms) if n_lms else max(30, kmax + 8)
    assert M >= kmax + 2
    p = np.arange(N)
    truth = np.stack([0.8 * p, 2.0 * np.sin(0.11 * p), 0.4 * np.sin(0.07 * p + 0.3)], axis=1)
    lms_true = np.stack([rng.uniform(-4, 0.8 * N + 4, M), rng.uniform(-9, 9, M)], axis=1)
    pose_est = truth + rng.normal(0, 0.03, (N, 3)) * [1, 1, 0.2]; lm_est = lms_true + rng.normal(0, 0.03, (M, 2))
    PW = 64 // max(T, 1) if T else 8
    WIDE, FIXED = 0, 1
    counts = counts_for(N, kmax, T or 8, full)
    wide_poses = [t * PW + 1 for t in range(3) if t * PW + 1 < N]
    seer = 5 if N > 5 else N - 1                                                # a free pose that sees the fixed landmark
    for a in wide_poses + [seer]:
        counts[a] = max(counts[a], 1)
    pl_p, pl_l = [], []
    for q in range(N):
        m = int(counts[q]); dup = q == 2 and kmax >= 2
        want = m - 1 if dup else m
        ls = []
        if q in (0, seer):
            ls.append(FIXED)
        if q in wide_poses and len(ls) < want:
            ls.append(WIDE)
        t = 0
        while len(ls) < want:
            l = (q * stride + t) % M; t += 1
            if l not in ls:
                ls.append(l)
        if dup:
            ls.append(ls[0])
        pl_p += [q] * len(ls); pl_l += ls
    pl_p = np.array(pl_p, dtype=np.int32); pl_l = np.array(pl_l, dtype=np.int32)

    def rel_pl(P, L):
        c, s = np.cos(P[:, 2]), np.sin(P[:, 2]); d = L - P[:, :2]
        return np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1]], axis=1)
    pl_z = rel_pl(truth[pl_p], lms_true[pl_l]) + rng.normal(0, 0.02, (len(pl_p), 2))
    pl_info = np.stack([_spd2(rng, 1e-3 if k % 9 == 4 else 1.0) for k in range(len(pl_p))])
    # odometry: the chain, then edges at the hub until it has max(5, T + 1) incidences (the first from the fixed pose 0, directions alternate)
    hub = N // 2; need = max(5, (T or 8) + 1)
    pp = [(i, i + 1) for i in range(N - 1)]
    others = [0] + [q for d in (7, 5, 11, 9, 13, 15, 17, 19) for q in (hub - d, hub + d) if 0 < q < N and abs(q - hub) > 1]
    if len(others) < need - 2:
        others = others + [q for q in range(N) if abs(q - hub) > 1]              # fewer poses than that: parallel edges, other direction
    for t, q in enumerate(others[:need - 2]):
        pp.append((q, hub) if t % 2 == 0 else (hub, q))
    pp_i = np.array([a for a, _ in pp], dtype=np.int32); pp_j = np.array([b for _, b in pp], dtype=np.int32)
    xi, xj = truth[pp_i], truth[pp_j]
    c, s = np.cos(xi[:, 2]), np.sin(xi[:, 2]); d = xj[:, :2] - xi[:, :2]
    pp_z = np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1], xj[:, 2] - xi[:, 2]], axis=1) + rng.normal(0, 0.01, (len(pp), 3)) * [1, 1, 0.3]
    pp_info = np.stack([_spd3(rng, 1e-3 if k % 11 == 5 else 1.0) for k in range(len(pp))])
    kernels = None
    if robust:                                                                   # a few gross outliers: wrong cone, slipped odometry
        pl_z[5::37] += [2.5, -1.5]; pp_z[7::29] += [0.8, -0.5, 0.1]
    if far:
        pose_est[:, :2] += FAR; lm_est += FAR
    g = dict(pose_est=pose_est, lm_est=lm_est, pp_i=pp_i, pp_j=pp_j, pp_z=pp_z, pp_info=pp_info, pl_p=pl_p, pl_l=pl_l, pl_z=pl_z, pl_info=pl_info,
             fixed_poses=np.array([0], dtype=np.int32), fixed_landmarks=np.array([FIXED], dtype=np.int32))
    if robust:
        kernels = {"observation": ("cauchy", _clear_delta(rr.edge_s(g, pose_est, lm_est)[1])), "odometry": ("huber", _clear_delta(rr.edge_s(g, pose_est, lm_est)[0]))}
    return g, kernels, dict(hub=hub, hub_incidences=need, wide=WIDE, wide_poses=wide_poses, counts=counts)


def _clear_delta(s):
    """delta with delta^2 in the widest gap between neighbours of the sorted s around their median: both branches of Huber get edges and no
    edge is near the branch point (lin_exact_ref asserts 1e-6 relative)"""
    v = np.sort(s); m = len(v) // 2; lo, hi = max(m - 3, 0), min(m + 3, len(v) - 1)
    k = lo + int(np.argmax(np.diff(v[lo:hi + 1])))
    d2 = 0.5 * (v[k] + v[k + 1])
    assert min(d2 - v[k], v[k + 1] - d2) > 1e-4 * d2
    return float(np.sqrt(d2))


def _case(T, kmax, **kw):
    d = dict(T=T, kmax=kmax, N=70, groups=None); d.update(kw)
    d["R"] = -(-kmax // (T or 8)); d["fallback"] = d["R"] > LIN_R
    return d


CASES = {}
for _k in (1, 2, 3, 4):
    CASES["t1_r%d" % _k] = _case(1, _k)
CASES["t1_tiles3"] = _case(1, 3, N=134)                                          # three wave tiles at T = 1, 6 live lanes in the last
CASES["t1_groups"] = _case(1, 4, n_lms=300, full=True, stride=4, groups="loop")            # > 25 groups: the loop from lane + 128
CASES["t1_groups12"] = _case(1, 4, n_lms=10, groups="first")                               # <= 12: the first item round only
CASES["t1_groups13to25"] = _case(1, 4, n_lms=20, groups="both")                            # 13 .. 25: both item rounds, not the loop
for _T, _ks in ((2, (2, 4, 5, 8)), (4, (4, 8, 9, 16)), (8, (16, 17, 32))):                   # R = 1 .. 4 at every T (T = 8, R = 1: auto_k8)
    for _k in _ks:
        CASES["t%d_k%d" % (_T, _k)] = _case(_T, _k)
CASES["auto_k8"] = _case(0, 8, full=True)
for _T, _k in ((1, 5), (2, 9), (4, 17), (8, 33)):
    CASES["t%d_k%d" % (_T, _k)] = _case(_T, _k)                                             # R = 5 > LIN_R: the gather kernels
for _T in (1, 2, 4, 8):
    CASES["far_t%d" % _T] = _case(_T, 2 * _T, far=True, seed=1)
CASES["n_lt_tile"] = _case(1, 2, N=5, full=True)
for _T in (1, 2, 4, 8):
    CASES["robust_t%d" % _T] = _case(_T, 3 * _T, robust=True, seed=2)
    for _R in (1, 2, 4):
        CASES["robust_t%d_r%d" % (_T, _R)] = _case(_T, _R * _T, robust=True, seed=3)

_built = {}


def graph(name):
    """(graph dict, kernels or None, notes) of a case; built once per process, never changed by a test"""
    if name not in _built:
        c = CASES[name]
        _built[name] = make(N=c["N"], kmax=c["kmax"], T=c["T"], n_lms=c.get("n_lms"), full=c.get("full", False), stride=c.get("stride", 7),
                            seed=c.get("seed", 0), far=c.get("far", False), robust=c.get("robust", False))
    return _built[name]


def handle_kw(name, gather=False):
    """keyword arguments of pkg.Graph for the case: the forced lanes, the robust kernels, the gather kernels on request"""
    c = CASES[name]; _, kernels, _ = graph(name)
    kw = dict(debug=dict(ell_lanes=c["T"]))
    if gather:
        kw["linearize_gather"] = 1
    for kind, (kname, delta) in (kernels or {}).items():
        kw["%s_robust_kernel" % kind] = kname; kw["%s_robust_delta" % kind] = delta
    return kw
