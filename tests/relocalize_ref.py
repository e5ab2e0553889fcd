"""Relocalisation restated in numpy float64 (TEST-ONLY), operation by operation from include/graphslam.h ("relocalisation") — not from the
kernels — and a second, independent checker that does not replay the search.

THE REFERENCE (run).  Every + - * / sqrt below is one IEEE fp64 operation in the order the header writes it; numpy rounds each ufunc on its own
(no contraction), division and sqrt are correctly rounded on both sides, so given the SAME z (the device's own, read back from
gs_polar_to_xy_batch) the device must return the same bits in everything the rule forms with those operations: tx, ty, count, cost, seed,
second_count, the runner-up's tx and ty, n_seeds, status, index, e2.  The one libm call is the final atan2(s, c).  THETA_ULPS states what it is
held to: DESIGN 22 counts a device libm call as 4 u |result| and doubles the total (8 u |theta|), and numpy.arctan2 (the host's libm) is
within one ulp = 2 u |theta| of the exact value itself: |theta_device - numpy.arctan2(s, c)| <= 10 u |theta|, u = 2^-53, with s and c the
reference's own (bitwise the device's when the winner is the same seed).  Nothing is fitted to a device output.

How the reference gets there differs from the device on purpose: it forms the whole n_map x n_map length matrix, screens it with a band that is
far wider than any rounding (2 length_tol + 1e-6 L around the frame's shortest and longest pair), applies the rule's own tests to what is left,
scores every seed against every cone by a dense distance matrix (argmin takes the lowest index among equal minima), and takes the smallest
key by a lexicographic sort.

THE CHECKER (check_truth).  Scenes are synthesised from a known pose with exact observations (relocalize_shapes): the returned pose must lie
within inlier_radius of the truth (position; the heading within inlier_radius / the farthest observation) and index must equal the truth's
matches.  It never enumerates a seed."""
import numpy as np

U = 2.0 ** -53
THETA_ULPS = 10.0                                                               # in units of u |theta| (see above)
INF = float("inf")
DEFAULTS = dict(seed_obs=12, min_inliers=4, min_baseline=2.0, length_tol=0.3, inlier_radius=0.5, type_tol=1e-4, distinct_xy=2.0,
                distinct_cos=0.98006657784124163)


def params_of(**kw):
    p = dict(DEFAULTS); p.update(kw)
    return p


def _score(c, s, tx, ty, zx, zy, zt, valid, map_xy, map_ty, p, want_index=False):
    """count [S], cost [S] of the seeds (c, s, t) [S]; with want_index the (index, e2) per observation of ONE seed"""
    S = len(c); R2 = p["inlier_radius"] * p["inlier_radius"]
    count = np.zeros(S, dtype=np.int64); cost = np.zeros(S)
    index = np.full(len(zx), -1, dtype=np.int32); e2o = np.full(len(zx), INF)
    lx, ly = map_xy[:, 0][None, :], map_xy[:, 1][None, :]
    with np.errstate(all="ignore"):
        for i in range(len(zx)):
            if not valid[i]:
                continue
            wx = (c * zx[i] - s * zy[i]) + tx; wy = (s * zx[i] + c * zy[i]) + ty
            ok = np.abs(map_ty.astype(np.float64) - zt[i]) < p["type_tol"]
            for lo in range(0, S, 4096):                                         # (memory)
                hi = min(S, lo + 4096)
                ex = lx - wx[lo:hi, None]; ey = ly - wy[lo:hi, None]
                e2 = ex * ex + ey * ey
                e2 = np.where(ok[None, :] & (e2 < R2), e2, INF)
                if e2.shape[1] == 0:
                    continue
                j = np.argmin(e2, axis=1); m = e2[np.arange(hi - lo), j]
                inl = m < INF
                count[lo:hi] += inl
                cost[lo:hi] = cost[lo:hi] + np.where(inl, m, 0.0)                # + 0.0 leaves a sum's bits as they are
                if want_index and inl[0]:
                    index[i] = j[0]; e2o[i] = m[0]
    return count, cost, index, e2o


def _frame(zx, zy, zt, base, map_xy, map_ty, M, p):
    """one frame: z (its observations' CoG-frame XY), zt (types), base (the position of its first observation in the call's arrays)"""
    k = len(zx); n_map = len(map_ty)
    none = dict(pose=np.zeros(3), c=0.0, s=0.0, count=0, cost=INF, seed=np.full(4, -1, dtype=np.int32), second_count=0, second_pose=np.zeros(3),
                n_seeds=0, status=2, index=np.full(k, -1, dtype=np.int32), e2=np.full(k, INF), second_cs=(0.0, 0.0))
    with np.errstate(all="ignore"):
        r2 = zx * zx + zy * zy
        valid = np.isfinite(zx) & np.isfinite(zy) & (r2 > 0.0)
    ids = [i for i in range(k) if valid[i]]
    ids.sort(key=lambda i: (r2[i], i))
    seeds = sorted(ids[:p["seed_obs"]])
    pairs = []
    for a in range(len(seeds)):
        for b in range(a + 1, len(seeds)):
            u, v = seeds[a], seeds[b]
            dzx = zx[v] - zx[u]; dzy = zy[v] - zy[u]
            L2 = dzx * dzx + dzy * dzy; L = np.sqrt(L2)
            if L >= p["min_baseline"]:
                pairs.append((u, v, dzx, dzy, L2, L))
    if not pairs or n_map < 2:
        return none
    # the screen: far wider than any rounding of M - L
    lmin = min(t[5] for t in pairs); lmax = max(t[5] for t in pairs); tol = p["length_tol"]
    with np.errstate(all="ignore"):
        band = (M >= lmin - 2.0 * tol - 1e-6 * lmin) & (M <= lmax + 2.0 * tol + 1e-6 * lmax)
    np.fill_diagonal(band, False)
    cp, cq = np.nonzero(band)                                                     # ordered pairs (p, q), p != q
    mt = map_ty.astype(np.float64)
    rows = []                                                                     # per seed: u, v, p, q, c, s, tx, ty
    with np.errstate(all="ignore"):
        for (u, v, dzx, dzy, L2, L) in pairs:
            Mc = M[cp, cq]
            hit = (np.abs(mt[cp] - zt[u]) < p["type_tol"]) & (np.abs(mt[cq] - zt[v]) < p["type_tol"]) & (np.abs(Mc - L) <= tol)
            pp, qq = cp[hit], cq[hit]
            if len(pp) == 0:
                continue
            dlx = map_xy[qq, 0] - map_xy[pp, 0]; dly = map_xy[qq, 1] - map_xy[pp, 1]
            M2 = dlx * dlx + dly * dly
            den = np.sqrt(L2 * M2)
            c = (dzx * dlx + dzy * dly) / den
            s = (dzx * dly - dzy * dlx) / den
            mzx = 0.5 * (zx[u] + zx[v]); mzy = 0.5 * (zy[u] + zy[v])
            mlx = 0.5 * (map_xy[pp, 0] + map_xy[qq, 0]); mly = 0.5 * (map_xy[pp, 1] + map_xy[qq, 1])
            tx = mlx - (c * mzx - s * mzy); ty = mly - (s * mzx + c * mzy)
            ex = (den > 0.0) & np.isfinite(c) & np.isfinite(s) & np.isfinite(tx) & np.isfinite(ty)
            if ex.any():
                n = int(ex.sum())
                rows.append((np.full(n, base + u), np.full(n, base + v), pp[ex], qq[ex], c[ex], s[ex], tx[ex], ty[ex]))
    if not rows:
        return none
    su, sv, sp, sq, c, s, tx, ty = (np.concatenate([r[t] for r in rows]) for t in range(8))
    count, cost, _, _ = _score(c, s, tx, ty, zx, zy, zt, valid, map_xy, map_ty, p)
    order = np.lexsort((sq, sp, sv, su, cost, -count))                            # the key (-count, cost, u, v, p, q), the last key first
    w = order[0]
    out = dict(none)
    out.update(c=float(c[w]), s=float(s[w]), count=int(count[w]), cost=float(cost[w]), seed=np.array([su[w], sv[w], sp[w], sq[w]], dtype=np.int32),
               n_seeds=len(c), status=0 if count[w] >= p["min_inliers"] else 1, pose=np.array([tx[w], ty[w], np.arctan2(s[w], c[w])]))
    _, _, out["index"], out["e2"] = _score(c[w:w + 1], s[w:w + 1], tx[w:w + 1], ty[w:w + 1], zx, zy, zt, valid, map_xy, map_ty, p, want_index=True)
    with np.errstate(all="ignore"):
        dx = tx - tx[w]; dy = ty - ty[w]
        near = ((dx * dx + dy * dy) < p["distinct_xy"] * p["distinct_xy"]) & ((c * c[w] + s * s[w]) > p["distinct_cos"])
    far = order[~near[order]]
    if len(far):
        r = far[0]
        out.update(second_count=int(count[r]), second_pose=np.array([tx[r], ty[r], np.arctan2(s[r], c[r])]), second_cs=(float(c[r]), float(s[r])))
    return out


def run(z, ty, frame_start, map_xy, map_ty, **params):
    """every frame's record (a list of dicts) from the observations' CoG-frame XY z [n, 2] and types ty [n]"""
    p = params_of(**params)
    z = np.asarray(z, dtype=np.float64).reshape(-1, 2); ty = np.asarray(ty, dtype=np.float64)
    map_xy = np.asarray(map_xy, dtype=np.float64).reshape(-1, 2); map_ty = np.asarray(map_ty, dtype=np.int32)
    with np.errstate(all="ignore"):
        dlx = map_xy[None, :, 0] - map_xy[:, None, 0]; dly = map_xy[None, :, 1] - map_xy[:, None, 1]      # [p, q] = l_q - l_p
        M = np.sqrt(dlx * dlx + dly * dly)
    out = []
    for f in range(len(frame_start) - 1):
        a, b = int(frame_start[f]), int(frame_start[f + 1])
        out.append(_frame(z[a:b, 0].copy(), z[a:b, 1].copy(), ty[a:b], a, map_xy, map_ty, M, p))
    return out


def theta_bound(theta):
    return THETA_ULPS * U * abs(theta)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def failures(ref, rec, f, index, e2, second=True):
    """what of frame f of a call's record (binding layout) and of its observations' index / e2 differs from the reference's frame `ref`"""
    bad = []
    def same(name, got, want):
        if not np.array_equal(_bits(np.asarray(got)), _bits(np.asarray(want, dtype=np.asarray(got).dtype))):
            bad.append("%s: %r, reference %r" % (name, got, want))
    same("status", rec["status"][f], ref["status"]); same("count", rec["count"][f], ref["count"]); same("cost", rec["cost"][f], ref["cost"])
    same("seed", rec["seed"][f], ref["seed"]); same("n_seeds", rec["n_seeds"][f], ref["n_seeds"])
    same("pose xy", rec["pose"][f][:2], ref["pose"][:2])
    if not abs(rec["pose"][f][2] - ref["pose"][2]) <= theta_bound(ref["pose"][2]):
        bad.append("theta: %r, numpy.arctan2 %r" % (rec["pose"][f][2], ref["pose"][2]))
    if second:
        same("second_count", rec["second_count"][f], ref["second_count"]); same("second pose xy", rec["second_pose"][f][:2], ref["second_pose"][:2])
        if not abs(rec["second_pose"][f][2] - ref["second_pose"][2]) <= theta_bound(ref["second_pose"][2]):
            bad.append("second theta: %r, numpy.arctan2 %r" % (rec["second_pose"][f][2], ref["second_pose"][2]))
    same("index", index, ref["index"]); same("e2", e2, ref["e2"])
    return bad


def check_truth(pose, index, truth_pose, truth_index, z, inlier_radius):
    """the independent checker: the pose within inlier_radius of the truth, the heading within inlier_radius / the farthest valid observation,
    index the truth's matches.  Returns the list of what fails."""
    bad = []
    pose = np.asarray(pose, dtype=np.float64); truth_pose = np.asarray(truth_pose, dtype=np.float64); z = np.asarray(z, dtype=np.float64).reshape(-1, 2)
    if not np.hypot(pose[0] - truth_pose[0], pose[1] - truth_pose[1]) < inlier_radius:
        bad.append("position %r is not within %g of %r" % (pose[:2], inlier_radius, truth_pose[:2]))
    r = np.sqrt((z * z).sum(1)); r = r[np.isfinite(r)]
    dth = np.arctan2(np.sin(pose[2] - truth_pose[2]), np.cos(pose[2] - truth_pose[2]))
    if not abs(dth) < inlier_radius / max(r.max() if len(r) else 1.0, 1.0):
        bad.append("heading %r is not within %g of %r" % (pose[2], inlier_radius / max(r.max() if len(r) else 1.0, 1.0), truth_pose[2]))
    if not np.array_equal(np.asarray(index, dtype=np.int64), np.asarray(truth_index, dtype=np.int64)):
        bad.append("index %r, the truth's matches %r" % (list(index), list(truth_index)))
    return bad
