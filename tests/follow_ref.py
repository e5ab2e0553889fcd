"""The reference of frame following (TEST-ONLY), written from include/graphslam.h ("frame following") — not from the kernels.

THE PREDICTION has one device libm call, sincos(theta); everything else is + - * in the header's order.  theta- = normalize_theta(theta + utheta)
has no libm at all: `normalize` below repeats it in float64 and the device's theta- is held to its BITS.  x-, y- and the six covariance entries
are carried as assoc_nn_ref.E pairs (exact value in mpmath, first-order error e), by that module's rules and the project's convention:
    c, s              sincos(theta)                                   e = 4 u |c|, 4 u |s|
    p = c ux - s uy   products 1 each, subtraction 1                  product rule, sum rule          (q = s ux + c uy likewise)
    x- = x + p        addition 1                                      e = e_p + u |x-|                (y- likewise)
    a = -q, b = p     exact
    S00 = (P00 + a P02) + a (P02 + a P22)   ...                       product and sum rules, one per operation of the header's line
    N00 = c (c q00 - s q01) - s (c q01 - s q11)   ...                 likewise
    Sigma- = S + N    addition 1 each
    product rule   e(a b) = |a| e_b + |b| e_a + u |a b|;   sum rule   e(a + b) = e_a + e_b + u |a + b|;   B = 2 e (the total doubled)
u = 2^-53.  Inputs (the state's pose and covariance, u, Qu) are the fp64 numbers the device holds, taken exactly.  Nothing here is fitted to a
device output.  `predict64` is the same formula in float64 (one ufunc per operation) for the replay; test_follow_cpu holds it to B as well.

THE UPDATE AND THE DUPLICATE PASS are additions and comparisons: `update` repeats them in float64 and is held bit for bit.

THE REPLAY (`replay`) runs whole sequences in plain float64 for the CPU tests: predict64, then per hypothesis the nearest admissible cone inside
the gate (assoc_nn_ref's formulas in float64; it REFUSES a frame in which two observations claim one cone — the scenes it is for are built
uncontested, where nearest is also minimum-cost), no pruning (the scenes are built so that the joint test keeps every pair), the iterated
localisation by the header's "frame localisation" rule with numpy's 3x3 solve, then `update`."""
import numpy as np

import assoc_exec as ax
import assoc_nn_ref as nr

E, U, MP, mpf = nr.E, nr.U, nr.MP, nr.mpf
PI = 3.14159265358979323846
UP = (0, 1, 2, 4, 5, 8)                                                        # the upper triangle's places in a row-major 3x3
MIRROR = (0, 1, 2, 1, 4, 5, 2, 5, 8)
TRACKING, LOST, DUPLICATE = 0, 1, 2
DEFAULTS = dict(min_pairs=3, max_misses=3, merge_xy=0.5, merge_theta=0.1)


def params_of(**kw):
    p = dict(DEFAULTS); p.update(kw)
    return p


def normalize(th):
    """g2o's normalize_theta as gs_iterate has it (the floor form), in float64: bit for bit the device's"""
    th = np.float64(th)
    if th >= -PI and th < PI:
        return th
    m = np.floor(th / np.float64(2.0 * PI))
    th = th - m * 2.0 * PI
    if th >= PI:
        th = th - 2.0 * PI
    if th < -PI:
        th = th + 2.0 * PI
    return np.float64(th)


def mirror(cov):
    """a 3x3 (9 values, upper triangle read) with its upper triangle mirrored; None: zeros"""
    return np.zeros(9) if cov is None else np.asarray(cov, dtype=np.float64).reshape(9)[list(MIRROR)]


def _predict(pose, cov9, u, qu, num):
    """the header's lines over `num` = (lift, cs): lift makes a number of the arithmetic, cs returns (c, s) of theta"""
    lift, cs = num
    x, y = lift(pose[0]), lift(pose[1]); c, s = cs(pose[2]); ux, uy = lift(u[0]), lift(u[1])
    p = (c * ux) - (s * uy); q = (s * ux) + (c * uy)
    xm = x + p; ym = y + q
    a = -q if num is F64 else q.neg(); b = p
    P00, P01, P02, P11, P12, P22 = (lift(cov9[t]) for t in UP)
    S = [(P00 + a * P02) + a * (P02 + a * P22), (P01 + a * P12) + b * (P02 + a * P22), P02 + a * P22,
         (P11 + b * P12) + b * (P12 + b * P22), P12 + b * P22, P22]
    if qu is not None:
        q00, q01, q02, q11, q12, q22 = (lift(qu[t]) for t in UP)
        N = [c * (c * q00 - s * q01) - s * (c * q01 - s * q11), s * (c * q00 - s * q01) + c * (c * q01 - s * q11), c * q02 - s * q12,
             s * (s * q00 + c * q01) + c * (s * q01 + c * q11), s * q02 + c * q12, q22]
    else:
        N = [lift(0.0)] * 6
    out = [S[t] + N[t] for t in range(6)]
    return xm, ym, out


F64 = (np.float64, lambda th: (np.cos(np.float64(th)), np.sin(np.float64(th))))


def _cs_exact(th):
    t = mpf(float(th)); cv, sv = MP.cos(t), MP.sin(t)
    return E(cv, 4 * U * abs(cv)), E(sv, 4 * U * abs(sv))


EXACT = (E, _cs_exact)


def predict64(pose, cov9, u, qu=None):
    """(prior pose [3], prior cov [9] mirrored) in float64"""
    with np.errstate(all="ignore"):
        xm, ym, S = _predict(pose, cov9, u, qu, F64)
        th = normalize(np.float64(pose[2]) + np.float64(u[2]))
    full = np.array([S[0], S[1], S[2], S[1], S[3], S[4], S[2], S[4], S[5]], dtype=np.float64)
    return np.array([xm, ym, th], dtype=np.float64), full


def predict_exact(pose, cov9, u, qu=None):
    """(x-, y- as E, theta- as float64 bits, the six upper-triangle entries as E): exact values and first-order errors; B = 2 e"""
    xm, ym, S = _predict(pose, cov9, u, qu, EXACT)
    return xm, ym, normalize(np.float64(pose[2]) + np.float64(u[2])), S


def inside(dev, ref):
    """|dev - exact| <= B = 2 e, and how much of B it takes (0 where both are exact and equal)"""
    d = abs(mpf(float(dev)) - ref.v); B = 2 * ref.e
    return d <= B, (float(d / B) if B > 0 else (0.0 if d == 0 else float("inf")))


# ---- the state and its update (bit for bit)
def new_state(poses, covs=None):
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3); nh = len(poses)
    cv = np.zeros((nh, 9)) if covs is None else np.stack([mirror(c) for c in np.asarray(covs, dtype=np.float64).reshape(-1, 9)])
    z = lambda: np.zeros(nh, dtype=np.int32)
    return dict(pose=poses.copy(), cov=cv, sum_chi2=np.zeros(nh), hits=z(), frames_hit=z(), frames_missed=z(), misses=z(), state=z(),
                state_step=np.full(nh, -1, dtype=np.int32), duplicate_of=np.full(nh, -1, dtype=np.int32))


def empty_record(prior_pose, prior_cov):
    """the chain's record of a step without a frame"""
    return dict(pose=np.array(prior_pose, dtype=np.float64), cov=np.array(prior_cov, dtype=np.float64), chi2=0.0, n_pairs=0, iterations=0, status=2, n_kept=0)


def update(st, t, priors, chain, gate, fp):
    """one step's update and duplicate pass ON st (in place).  priors[h] = (pose [3], cov [9]) and chain[h] = the chain's record (dict: pose, cov,
    chi2, n_pairs, iterations, status, n_kept) of every hypothesis that tracked before the step (others: ignored).  Returns the step records
    (a list of dicts with prior_pose, prior_cov, pose, cov, chi2, n_pairs, iterations, status, n_kept, accepted, state), best, n_tracking"""
    nh = len(st["state"]); recs = []
    merge2 = np.float64(fp["merge_xy"]) * np.float64(fp["merge_xy"])
    for h in range(nh):
        if st["state"][h] != TRACKING:
            recs.append(dict(prior_pose=st["pose"][h].copy(), prior_cov=st["cov"][h].copy(), pose=st["pose"][h].copy(), cov=st["cov"][h].copy(), chi2=0.0,
                             n_pairs=0, iterations=0, status=-1, n_kept=0, accepted=0, state=int(st["state"][h])))
            continue
        pp, pc = priors[h]; c = chain[h]; n_pairs = int(c["n_pairs"])
        ok = c["status"] <= 1 and n_pairs >= fp["min_pairs"] and 0 <= n_pairs <= 256 and bool(np.float64(c["chi2"]) <= np.float64(gate[n_pairs]))
        if ok:
            st["pose"][h] = c["pose"]; st["cov"][h] = c["cov"]; st["hits"][h] += n_pairs; st["sum_chi2"][h] = st["sum_chi2"][h] + np.float64(c["chi2"])
            st["frames_hit"][h] += 1; st["misses"][h] = 0
        else:
            st["pose"][h] = pp; st["cov"][h] = pc; st["frames_missed"][h] += 1; st["misses"][h] += 1
            if st["misses"][h] >= fp["max_misses"]:
                st["state"][h] = LOST; st["state_step"][h] = t
        recs.append(dict(prior_pose=np.array(pp, dtype=np.float64), prior_cov=np.array(pc, dtype=np.float64), pose=np.array(c["pose"], dtype=np.float64),
                         cov=np.array(c["cov"], dtype=np.float64), chi2=float(c["chi2"]), n_pairs=n_pairs, iterations=int(c["iterations"]),
                         status=int(c["status"]), n_kept=int(c["n_kept"]), accepted=int(ok), state=None, _was=True))
    with np.errstate(all="ignore"):
        for h in range(1, nh):                                                 # the sequential rule
            if st["state"][h] != TRACKING:
                continue
            for d in range(h):
                if st["state"][d] != TRACKING:
                    continue
                dx = st["pose"][h, 0] - st["pose"][d, 0]; dy = st["pose"][h, 1] - st["pose"][d, 1]
                dth = normalize(st["pose"][h, 2] - st["pose"][d, 2]) if np.isfinite(st["pose"][h, 2] - st["pose"][d, 2]) else np.nan
                if bool(((dx * dx) + (dy * dy)) < merge2) and bool(np.abs(dth) < np.float64(fp["merge_theta"])):
                    st["state"][h] = DUPLICATE; st["duplicate_of"][h] = d; st["state_step"][h] = t
                    break
    for h, r in enumerate(recs):
        if r.pop("_was", False):
            r["state"] = int(st["state"][h])
    return recs, best_of(st), int((st["state"] == TRACKING).sum())


REC_F = ("prior_pose", "prior_cov", "pose", "cov", "chi2")
REC_I = ("n_pairs", "iterations", "status", "n_kept", "accepted", "state")


def mismatches(dev, rec):
    """the fields in which a device step record (a FOLLOW_STEP row, or a dict) differs from one of `update`'s: doubles by their bits"""
    bad = [k for k in REC_F if np.asarray(dev[k], dtype=np.float64).tobytes() != np.asarray(rec[k], dtype=np.float64).tobytes()]
    return bad + [k for k in REC_I if int(dev[k]) != int(rec[k])]


def best_of(st):
    best = -1
    for h in range(len(st["state"])):
        if st["state"][h] != TRACKING:
            continue
        if best < 0 or st["hits"][h] > st["hits"][best] or (st["hits"][h] == st["hits"][best] and st["sum_chi2"][h] < st["sum_chi2"][best]):
            best = h
    return best


# ---- the replay's chain in float64
def _query(pose, z, prm, pc):
    c, s = np.cos(pose[2]), np.sin(pose[2])
    wx, wy = z[0] * c - z[1] * s, z[0] * s + z[1] * c
    r2 = z[0] * z[0] + z[1] * z[1]
    k = prm["sigma_range"] ** 2 / r2; sb2 = prm["sigma_bearing"] ** 2; sx2 = prm["sigma_xy"] ** 2
    A = np.array([[k * wx * wx + sb2 * wy * wy + sx2, k * wx * wy - sb2 * wx * wy], [0.0, k * wy * wy + sb2 * wx * wx + sx2]]); A[1, 0] = A[0, 1]
    wp = np.array([-wy, wx])
    if pc is not None:
        G = np.array([[1.0, 0.0, wp[0]], [0.0, 1.0, wp[1]]]); A = A + G @ np.asarray(pc).reshape(3, 3) @ G.T
    return np.array([wx + pose[0], wy + pose[1]]), A, wp, r2


def assign64(pose, cov9, obs, map_xy, map_ty, map_cov, prm):
    """index [k] (-1: none) and d2 [k]: the nearest admissible cone of every observation; refuses a contested frame"""
    z = ax.polar_to_xy(obs[:, 0], obs[:, 1], obs[:, 2], prm["lidar"]); idx = np.full(len(obs), -1, dtype=np.int32); d2o = np.full(len(obs), np.inf)
    with np.errstate(all="ignore"):
        for i in range(len(obs)):
            g, A, _, r2 = _query(pose, z[i], prm, cov9)
            if not (np.isfinite(g).all() and r2 > 0.0):
                continue
            for j in np.nonzero(np.abs(map_ty - obs[i, 3]) < prm["type_tol"])[0]:
                nu = map_xy[j] - g
                if not np.sqrt(nu @ nu) < prm["max_distance"]:
                    continue
                S = A + (np.zeros((2, 2)) if map_cov is None else np.asarray(map_cov[j]).reshape(2, 2))
                det = S[0, 0] * S[1, 1] - S[0, 1] * S[0, 1]
                d2 = (S[1, 1] * nu[0] * nu[0] - 2.0 * S[0, 1] * nu[0] * nu[1] + S[0, 0] * nu[1] * nu[1]) / det
                if det > 0.0 and S[0, 0] > 0.0 and d2 < prm["gate_chi2"] and d2 < d2o[i]:
                    idx[i] = j; d2o[i] = d2
    taken = idx[idx >= 0]
    assert len(set(taken.tolist())) == len(taken), "the replay is for uncontested frames: two observations claim one cone"
    return idx, d2o


def localize64(pose, cov9, obs, idx, map_xy, map_cov, prm, loc):
    """the header's iterated localisation in float64: dict(pose, cov, chi2, n_pairs, iterations, status)"""
    P = np.asarray(cov9, dtype=np.float64).reshape(3, 3); x0 = np.asarray(pose, dtype=np.float64)
    z = ax.polar_to_xy(obs[:, 0], obs[:, 1], obs[:, 2], prm["lidar"]); rows = [i for i in range(len(obs)) if idx[i] >= 0]

    def sums(x):
        a = 0.0; c = np.zeros(3); M = np.zeros((3, 3)); m = 0
        with np.errstate(all="ignore"):
            for i in rows:
                g, Q, wp, r2 = _query(x, z[i], prm, None); j = idx[i]
                D = Q + (np.zeros((2, 2)) if map_cov is None else np.asarray(map_cov[j]).reshape(2, 2)); nu = map_xy[j] - g
                det = D[0, 0] * D[1, 1] - D[0, 1] * D[0, 1]
                if not (np.isfinite(g).all() and r2 > 0.0 and det > 0.0 and D[0, 0] > 0.0 and np.isfinite(nu).all()):
                    continue
                Ei = np.array([[D[1, 1], -D[0, 1]], [-D[0, 1], D[0, 0]]]) / det; J = np.array([[1.0, 0.0, wp[0]], [0.0, 1.0, wp[1]]])
                a += nu @ Ei @ nu; c += J.T @ Ei @ nu; M += J.T @ Ei @ J; m += 1
        return a, c, M, m

    d = np.zeros(3); x = np.zeros(3); iters = 0; status = 1
    for it in range(loc["max_iterations"]):
        _, c, M, m = sums(x0 + d if it else x0)
        if it == 0 and m == 0:
            return dict(pose=x0.copy(), cov=P.reshape(9).copy(), chi2=0.0, n_pairs=0, iterations=0, status=2)
        b = c + M @ d if it else c
        x = np.linalg.solve(np.eye(3) + M @ P, b); dn = P @ x; iters += 1
        if not np.isfinite(dn).all():
            return dict(pose=x0.copy(), cov=P.reshape(9).copy(), chi2=np.inf, n_pairs=0, iterations=iters, status=3)
        conv = abs(dn[0] - d[0]) <= loc["tol_xy"] and abs(dn[1] - d[1]) <= loc["tol_xy"] and abs(dn[2] - d[2]) <= loc["tol_theta"]
        d = dn
        if conv:
            status = 0
            break
    a, _, M, m = sums(x0 + d)
    cov = P @ np.linalg.inv(np.eye(3) + M @ P); cov = 0.5 * (cov + cov.T)
    xf = x0 + d; xf[2] = normalize(xf[2])
    return dict(pose=xf, cov=cov.reshape(9), chi2=float(a + x @ d), n_pairs=m, iterations=iters, status=status)


def replay(poses, covs, frames, motion, motion_cov, map_xy, map_ty, map_cov, prm, gate, loc, fp):
    """a whole run in float64: (steps [t][h] as update's records plus d2 = the assignment's distances, final state, best, n_tracking)"""
    st = new_state(poses, covs); steps = []; best, nt = best_of(st), len(st["state"])
    for t, obs in enumerate(frames):
        obs = np.asarray(obs, dtype=np.float64).reshape(-1, 4); priors, chain, d2s = {}, {}, {}
        for h in range(len(st["state"])):
            if st["state"][h] != TRACKING:
                continue
            if t == 0:
                pp, pc = st["pose"][h].copy(), st["cov"][h].copy()
            else:
                pp, pc = predict64(st["pose"][h], st["cov"][h], motion[t - 1], None if motion_cov is None else motion_cov[t - 1])
            priors[h] = (pp, pc)
            if len(obs) == 0:
                chain[h] = empty_record(pp, pc); d2s[h] = np.zeros(0)
                continue
            idx, d2 = assign64(pp, pc, obs, map_xy, map_ty, map_cov, prm)
            r = localize64(pp, pc, obs, idx, map_xy, map_cov, prm, loc); r["n_kept"] = int((idx >= 0).sum())
            chain[h] = r; d2s[h] = d2
        recs, best, nt = update(st, t, priors, chain, gate, fp)
        for h, r in enumerate(recs):
            r["d2"] = d2s.get(h)
        steps.append(recs)
    return steps, st, best, nt
