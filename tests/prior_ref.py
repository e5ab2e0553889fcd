"""Checker of the prior edges (gs_add_pose_prior / gs_add_pose_xy_prior / gs_add_landmark_prior) — numpy and the UNCHANGED CPU oracle.

The oracle has no unary edge and needs none: a pose prior (z, Omega) on pose p is the odometry edge (a -> p, z, Omega) from an
auxiliary FIXED pose a at exactly (0, 0, 0) — a^-1 o x adds zeros and multiplies by one, so the edge's error is vec(z^-1 o x) and its
Jacobian with respect to x is diag(R_z^T, 1) —, a landmark prior is the observation edge (a -> l, z, Omega), and an XY prior is the pose
prior with z_theta = 0 and Omega in the upper-left 2 x 2 of a 3 x 3 that is zero elsewhere.  augment() appends that one pose LAST and
the extra edges behind the graph's own; everything is then compared against OracleGraph / lm_ref on the augmented graph, with the
auxiliary vertex's rows dropped (strip).  A prior on a fixed vertex becomes an edge between two fixed vertices: inactive in the oracle.
With robust kernels the graph's own edges are re-weighted first (robust_ref.reweighted) and the prior edges appended at weight 1.
terms() is the same arithmetic in plain numpy, independent of the oracle: test_prior_cpu.py pins the two against each other.

A prior set: dict(pose=[(pose index, z[3], W[3, 3], xy)], lm=[(landmark index, z[2], W[2, 2])]) in insertion order; xy = True marks an
entry added through the XY call (z[2] = 0, W embedded)."""
import numpy as np

import robust_ref as rr


def embed_xy(z2, W2):
    W = np.zeros((3, 3)); W[:2, :2] = np.asarray(W2, dtype=np.float64).reshape(2, 2)
    return np.array([z2[0], z2[1], 0.0]), W


def spd(rng, n, scale):
    A = rng.normal(size=(n, n)); S = A @ A.T + n * np.eye(n)
    return scale * (S + S.T) / 2


def prior_set(g, seed=0, every_pose=7, every_lm=5, s_pose=0.4, s_xy=0.3, s_lm=0.02, noise=0.2):
    """SE2 priors (z_theta != 0, full Omega) on about every 7th pose, XY priors on other poses, landmark priors on about every 5th cone
    that has an observation edge, TWO priors on one pose and on one cone, one prior on a fixed pose and one on a fixed cone (where the
    graph has one).  z = the graph's estimate + noise."""
    rng = np.random.default_rng(1000 + seed)
    P = np.asarray(g["pose_est"], dtype=np.float64); L = np.asarray(g["lm_est"], dtype=np.float64)
    N, M = len(P), len(L)
    fixed_p = set(int(i) for i in g["fixed_poses"]); fixed_l = set(int(i) for i in g["fixed_landmarks"])
    seen = np.bincount(np.asarray(g["pl_l"], dtype=np.int64), minlength=M) > 0
    pose, lm = [], []
    def se2(p):
        z = P[p] + rng.normal(0, noise, 3) * [1, 1, 0.2]
        pose.append((p, z, spd(rng, 3, s_pose), False))
    def xy(p):
        z, W = embed_xy(P[p, :2] + rng.normal(0, noise, 2), spd(rng, 2, s_xy)); pose.append((p, z, W, True))
    def lmp(l):
        lm.append((l, L[l] + rng.normal(0, noise, 2), spd(rng, 2, s_lm)))
    free_p = [p for p in range(N) if p not in fixed_p]
    for k, p in enumerate(free_p):
        if k % every_pose == 3: se2(p)
        elif k % 5 == 1: xy(p)
    free_l = [l for l in range(M) if l not in fixed_l and seen[l]]
    for k, l in enumerate(free_l):
        if k % every_lm == 2: lmp(l)
    dbl_p = free_p[3 if len(free_p) > 3 else 0]; xy(dbl_p); se2(dbl_p)              # a second and third prior on one pose (XY, then SE2)
    dbl_l = free_l[2 if len(free_l) > 2 else 0]; lmp(dbl_l)
    if fixed_p: se2(sorted(fixed_p)[0])
    if fixed_l: lmp(sorted(fixed_l)[0])
    return dict(pose=pose, lm=lm)


def add_to(G, pri, ids_pose=None, ids_lm=None):
    """the set into a handle, one call per prior, through the call it was made for (ids default: the indices)"""
    for p, z, W, is_xy in pri["pose"]:
        pid = int(p if ids_pose is None else ids_pose[p])
        if is_xy: G.add_pose_xy_prior(pid, z[:2], W[:2, :2])
        else: G.add_pose_prior(pid, z, W)
    for l, z, W in pri["lm"]:
        G.add_landmark_prior(int(l if ids_lm is None else ids_lm[l]), z, W)


def augment(g, pri, poses=None, lms=None):
    """the graph dict with the auxiliary fixed pose (index N, the last) and the prior edges behind the graph's own"""
    P = np.asarray(g["pose_est"] if poses is None else poses, dtype=np.float64).reshape(-1, 3)
    L = np.asarray(g["lm_est"] if lms is None else lms, dtype=np.float64).reshape(-1, 2)
    N = len(P)
    out = dict(g)
    out["pose_est"] = np.vstack([P, np.zeros((1, 3))]); out["lm_est"] = L.copy()
    np_, nl = len(pri["pose"]), len(pri["lm"])
    out["pp_i"] = np.concatenate([np.asarray(g["pp_i"], dtype=np.int32), np.full(np_, N, dtype=np.int32)])
    out["pp_j"] = np.concatenate([np.asarray(g["pp_j"], dtype=np.int32), np.array([p for p, _, _, _ in pri["pose"]], dtype=np.int32)])
    out["pp_z"] = np.vstack([np.asarray(g["pp_z"], dtype=np.float64).reshape(-1, 3)] + [np.reshape(z, (1, 3)) for _, z, _, _ in pri["pose"]])
    out["pp_info"] = np.vstack([np.asarray(g["pp_info"], dtype=np.float64).reshape(-1, 9)] + [np.reshape(W, (1, 9)) for _, _, W, _ in pri["pose"]])
    out["pl_p"] = np.concatenate([np.asarray(g["pl_p"], dtype=np.int32), np.full(nl, N, dtype=np.int32)])
    out["pl_l"] = np.concatenate([np.asarray(g["pl_l"], dtype=np.int32), np.array([l for l, _, _ in pri["lm"]], dtype=np.int32)])
    out["pl_z"] = np.vstack([np.asarray(g["pl_z"], dtype=np.float64).reshape(-1, 2)] + [np.reshape(z, (1, 2)) for _, z, _ in pri["lm"]])
    out["pl_info"] = np.vstack([np.asarray(g["pl_info"], dtype=np.float64).reshape(-1, 4)] + [np.reshape(W, (1, 4)) for _, _, W in pri["lm"]])
    out["fixed_poses"] = np.concatenate([np.asarray(g["fixed_poses"], dtype=np.int32), np.array([N], dtype=np.int32)])
    return out


def augment_robust(g, pri, P, L, kernels):
    """re-weight the graph's own edges at (P, L) FIRST, then append the prior edges at weight 1"""
    return augment(rr.reweighted(g, P, L, kernels), pri)


def strip(blocks, g):
    """the augmented oracle's blocks without the auxiliary pose's rows and the prior edges' (zero) off-diagonal blocks"""
    N, Epp, Epl = len(g["pose_est"]), len(g["pp_i"]), len(g["pl_p"])
    return dict(Hpp_diag=blocks["Hpp_diag"][:N], Hll_diag=blocks["Hll_diag"], Hpp_off=blocks["Hpp_off"][:Epp], Hpl=blocks["Hpl"][:Epl],
                b_pose=blocks["b_pose"][:N], b_lm=blocks["b_lm"])


def terms(pri, P, L):
    """plain numpy: per prior (e, J, J^T W J, -J^T W e, e^T W e), pose priors then landmark priors, insertion order"""
    out_p, out_l = [], []
    for p, z, W, _ in pri["pose"]:
        c, s = np.cos(z[2]), np.sin(z[2]); Rt = np.array([[c, s], [-s, c]])
        e = np.r_[Rt @ (P[p, :2] - z[:2]), rr.normalize_theta(P[p, 2] - z[2])]
        J = np.eye(3); J[:2, :2] = Rt
        out_p.append((e, J, J.T @ W @ J, -J.T @ W @ e, float(e @ W @ e)))
    for l, z, W in pri["lm"]:
        e = L[l] - z
        out_l.append((e, np.eye(2), np.array(W), -W @ e, float(e @ W @ e)))
    return out_p, out_l


def chi2_each(pri, P, L):
    tp, tl = terms(pri, np.asarray(P), np.asarray(L))
    return np.array([t[4] for t in tp]), np.array([t[4] for t in tl])


def contributions(g, pri, P, L):
    """what the priors on FREE vertices add: (Hpp_diag [N, 9], b_pose [N, 3], Hll_diag [M, 4], b_lm [M, 2], chi2), summed in insertion order"""
    P = np.asarray(P); L = np.asarray(L)
    N, M = len(P), len(L)
    fixed_p = set(int(i) for i in g["fixed_poses"]); fixed_l = set(int(i) for i in g["fixed_landmarks"])
    Hp = np.zeros((N, 9)); bp = np.zeros((N, 3)); Hl = np.zeros((M, 4)); bl = np.zeros((M, 2)); chi = 0.0
    tp, tl = terms(pri, P, L)
    for (p, _, _, _), (e, J, H, b, c) in zip(pri["pose"], tp):
        if p not in fixed_p:
            Hp[p] += H.reshape(9); bp[p] += b; chi += c
    for (l, _, _), (e, J, H, b, c) in zip(pri["lm"], tl):
        if l not in fixed_l:
            Hl[l] += H.reshape(4); bl[l] += b; chi += c
    return Hp, bp, Hl, bl, chi
