"""Checker of the robust kernels (numpy only): per-edge errors of EdgeSE2 / EdgeSE2PointXY in the oracle's operation order, the
squared error s = e^T Omega e, weight w = rho'(s) and rho(s) of the three kernels, and the re-weighted graph.

A robust linearisation at estimates x is the PLAIN linearisation of the same graph with every information matrix scaled by its
edge's weight at x — so everything else (H, b, the solve, the iterations) is checked with the existing CPU oracle on
`reweighted(...)`, unchanged.  test_robust_cpu.py pins the per-edge values below to OracleGraph.chi2() first.

Kernels (g2o RobustKernelHuber / RobustKernelCauchy, restated), d2 = delta^2:
    none    rho = s                                        w = 1
    huber   rho = s if s <= d2 else 2 sqrt(s) delta - d2   w = 1 if s <= d2 else delta / sqrt(s)
    cauchy  rho = d2 log(1 + s / d2)                       w = 1 / (1 + s / d2)
`kernels` everywhere: {"odometry": (name, delta), "observation": (name, delta)}; a missing kind means ("none", 1.0)."""
import numpy as np

NONE = ("none", 1.0)


def normalize_theta(th):
    th = np.array(th, dtype=np.float64, copy=True)
    out = ~((th >= -np.pi) & (th < np.pi))
    t = th[out]
    t = t - np.floor(t / (2 * np.pi)) * 2 * np.pi
    t = np.where(t >= np.pi, t - 2 * np.pi, t)
    t = np.where(t < -np.pi, t + 2 * np.pi, t)
    th[out] = t
    return th


def se2_inverse(a):
    th = normalize_theta(-a[:, 2]); c, s = np.cos(th), np.sin(th)
    tx, ty = -a[:, 0], -a[:, 1]
    return np.stack([c * tx - s * ty, s * tx + c * ty, th], axis=1)


def se2_compose(a, b):
    c, s = np.cos(a[:, 2]), np.sin(a[:, 2])
    return np.stack([a[:, 0] + (c * b[:, 0] - s * b[:, 1]), a[:, 1] + (s * b[:, 0] + c * b[:, 1]), normalize_theta(a[:, 2] + b[:, 2])], axis=1)


def errors_pp(g, poses):
    """[E,3] e = vec(z^-1 * (x_i^-1 * x_j))"""
    poses = np.asarray(poses, dtype=np.float64)
    xi, xj = poses[g["pp_i"]], poses[g["pp_j"]]
    return se2_compose(se2_inverse(np.asarray(g["pp_z"], dtype=np.float64).reshape(-1, 3)), se2_compose(se2_inverse(xi), xj))


def errors_pl(g, poses, lms):
    """[E,2] e = (x_p^-1 * l) - z"""
    poses = np.asarray(poses, dtype=np.float64); lms = np.asarray(lms, dtype=np.float64)
    inv = se2_inverse(poses[g["pl_p"]]); l = lms[g["pl_l"]]; z = np.asarray(g["pl_z"], dtype=np.float64).reshape(-1, 2)
    c, s = np.cos(inv[:, 2]), np.sin(inv[:, 2])
    return np.stack([(c * l[:, 0] - s * l[:, 1]) + inv[:, 0] - z[:, 0], (s * l[:, 0] + c * l[:, 1]) + inv[:, 1] - z[:, 1]], axis=1)


def edge_s(g, poses, lms):
    """(s_pp [Epp], s_pl [Epl]): e^T Omega e of every edge (edges between fixed vertices included)"""
    e = errors_pp(g, poses); W = np.asarray(g["pp_info"], dtype=np.float64).reshape(-1, 3, 3)
    s_pp = np.einsum("er,erc,ec->e", e, W, e)
    e = errors_pl(g, poses, lms); W = np.asarray(g["pl_info"], dtype=np.float64).reshape(-1, 2, 2)
    s_pl = np.einsum("er,erc,ec->e", e, W, e)
    return s_pp, s_pl


def rho(kernel, s):
    name, delta = kernel
    s = np.asarray(s, dtype=np.float64); d2 = delta * delta
    if name == "none":
        return s.copy()
    if name == "huber":
        r = np.sqrt(np.maximum(s, 0.0))
        return np.where(s <= d2, s, 2.0 * r * delta - d2)
    if name == "cauchy":
        return d2 * np.log(1.0 + s / d2)
    raise ValueError(name)


def weight(kernel, s):
    name, delta = kernel
    s = np.asarray(s, dtype=np.float64); d2 = delta * delta
    if name == "none":
        return np.ones_like(s)
    if name == "huber":
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(s <= d2, 1.0, delta / np.sqrt(np.maximum(s, 0.0)))
    if name == "cauchy":
        return 1.0 / (1.0 + s / d2)
    raise ValueError(name)


def active(g):
    """(a_pp, a_pl): edges that count in chi2 (not between two fixed vertices)"""
    pf = np.zeros(len(g["pose_est"]), dtype=bool); pf[np.asarray(g["fixed_poses"], dtype=np.int64)] = True
    lf = np.zeros(len(g["lm_est"]), dtype=bool); lf[np.asarray(g["fixed_landmarks"], dtype=np.int64)] = True
    return ~(pf[g["pp_i"]] & pf[g["pp_j"]]), ~(pf[g["pl_p"]] & lf[g["pl_l"]])


def robust_chi2(g, poses, lms, kernels):
    """sum of rho(s) over the active edges (g2o activeRobustChi2)"""
    s_pp, s_pl = edge_s(g, poses, lms); a_pp, a_pl = active(g)
    return float(rho(kernels.get("odometry", NONE), s_pp)[a_pp].sum() + rho(kernels.get("observation", NONE), s_pl)[a_pl].sum())


def reweighted(g, poses, lms, kernels):
    """copy of the graph dict with pp_info / pl_info rows multiplied by w at the given estimates, and those estimates"""
    s_pp, s_pl = edge_s(g, poses, lms)
    out = dict(g)
    out["pose_est"] = np.array(poses, dtype=np.float64, copy=True); out["lm_est"] = np.array(lms, dtype=np.float64, copy=True)
    out["pp_info"] = np.asarray(g["pp_info"], dtype=np.float64).reshape(-1, 9) * weight(kernels.get("odometry", NONE), s_pp)[:, None]
    out["pl_info"] = np.asarray(g["pl_info"], dtype=np.float64).reshape(-1, 4) * weight(kernels.get("observation", NONE), s_pl)[:, None]
    return out


def irls(po, g, kernels, iterations, make_oracle_graph, ordering=1, poses=None, lms=None):
    """Iteratively re-weighted Gauss-Newton with the oracle: rebuild the oracle graph from the re-weighted dict at the current
    estimates, one optimize(1), repeat.  Returns (poses, lms, chi[it]) with chi[it] = sum rho at the linearisation point of
    iteration it (what gs_optimize files per iteration), and the last increment (dpose, dlm)."""
    P = np.array(g["pose_est"] if poses is None else poses, dtype=np.float64, copy=True)
    L = np.array(g["lm_est"] if lms is None else lms, dtype=np.float64, copy=True)
    chi = []; delta = None
    for _ in range(iterations):
        chi.append(robust_chi2(g, P, L, kernels))
        og = make_oracle_graph(po, reweighted(g, P, L, kernels))
        done, _, _ = og.optimize(1, ordering=ordering)
        assert done == 1
        P, L = og.poses(), og.landmarks(); delta = og.delta()
    return P, L, np.array(chi), delta


def stop_iteration(chi, rel_tol, max_iterations):
    """updates gs_optimize_until applies given the sum-rho sequence at the linearisation points (the oracle's orc_optimize_until): the
    rule fires in the iteration whose chi2 differs from the previous one's by <= rel_tol * chi2; that iteration's update still goes in"""
    for it in range(1, min(len(chi), max_iterations)):
        if abs(chi[it - 1] - chi[it]) <= rel_tol * chi[it]:
            return it + 1
    return max_iterations


def median_deltas(g, poses, lms):
    """delta per kind = median of sqrt(s) of that kind at the given estimates (both Huber branches get edges)"""
    s_pp, s_pl = edge_s(g, poses, lms)
    return float(np.median(np.sqrt(s_pp))), float(np.median(np.sqrt(s_pl)))


def outlier_graph(g, x_poses, x_lms, seed, share=0.05, nearest=5, min_dist=3.0):
    """The bench graph with a seeded share of its observation edges re-targeted to one of the `nearest` cones at least `min_dist`
    metres from the right one (distances at the clean optimum); estimates = the clean optimum.  Returns (graph, outlier edge indices)."""
    rng = np.random.default_rng(seed)
    x_lms = np.asarray(x_lms, dtype=np.float64)
    E = len(g["pl_p"]); pick = np.sort(rng.choice(E, int(round(share * E)), replace=False))
    out = dict(g); pl_l = np.array(g["pl_l"], copy=True)
    for k in pick:
        d = np.hypot(*(x_lms - x_lms[pl_l[k]]).T)
        cand = np.flatnonzero(d >= min_dist); cand = cand[np.argsort(d[cand], kind="stable")][:nearest]
        pl_l[k] = cand[rng.integers(len(cand))]
    out["pl_l"] = pl_l.astype(np.int32)
    out["pose_est"] = np.array(x_poses, dtype=np.float64, copy=True); out["lm_est"] = np.array(x_lms, copy=True)
    return out, pick
