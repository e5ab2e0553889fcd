"""Checker of the polar observation edges (gs_add_range_bearing_edge / gs_add_bearing_edge) — numpy and the UNCHANGED CPU oracle.

With d = x_p^-1 * l, r = |d|, beta = atan2(dy, dx), a polar edge has e = (r - z_r, normalize_theta(beta - z_beta)) and the Jacobians
Jd = d(r, beta)/dd = [[dx/r, dy/r], [-dy/r^2, dx/r^2]], B = Jd R^T, A = Jd [-R^T | (dy, -dx)^T] = [-B | (0, -1)^T].  H does not depend
on e, so AT estimates (P, L) a polar edge with Jd evaluated there is — for H, b and chi2, exactly — the Cartesian edge with
    information Jd^T Omega Jd   and   measurement z' = d - Jd^-1 e      (e_r := 0 for bearing-only: Omega's range row is zero)
because that edge's error is d - z' = Jd^-1 e and its Jacobians are [-R^T | (dy, -dx)^T] and R^T.  cartesianised() rewrites the polar
edges that way; the oracle on that graph is the reference for the blocks, b, chi2 and ONE Gauss-Newton step, and iterations
re-cartesianise at every iterate (gauss_newton), as robust_ref.reweighted does for kernels.  Robust weights compose: reweighted() applied
to the cartesianised graph sees the same s.  terms() / contributions() are the same arithmetic in plain numpy, independent of the oracle:
test_polar_cpu.py pins the two against each other.  lm_run() restates lm_ref.run over this system_at (lm_ref.py stays as it is).

A polar set: dict(idx = observation-edge indices of the graph dict, ascending; model = 1 range-bearing / 2 bearing-only per entry;
z [n, 2] = (z_r, z_beta); W [n, 2, 2] = Omega in (range, bearing)).  The graph dict keeps its Cartesian edge at those indices (it is what
the polar measurement was taken from); a handle gets the polar edge in its place (load), so edge indices agree everywhere."""
import numpy as np

import lm_ref
import robust_ref as rr

RANGE_BEARING, BEARING = 1, 2


def polar_set(g, every_rb=3, every_b=7):
    """A third of the observation edges range-bearing, a seventh bearing-only; besides: every edge of one cone polar, every edge of one
    free pose polar, one polar edge on a fixed cone and one on a fixed pose (where the graph has them).  z from the Cartesian z;
    Omega_rr = W_00, Omega_rb = r W_01, Omega_bb = r^2 W_11 (r = z_r); bearing-only keeps Omega_bb."""
    pl_p = np.asarray(g["pl_p"], dtype=np.int64); pl_l = np.asarray(g["pl_l"], dtype=np.int64); E = len(pl_p)
    z = np.asarray(g["pl_z"], dtype=np.float64).reshape(-1, 2); W = np.asarray(g["pl_info"], dtype=np.float64).reshape(-1, 2, 2)
    model = np.zeros(E, dtype=np.int32)
    k = np.arange(E)
    model[k % every_rb == 1] = RANGE_BEARING
    model[(model == 0) & (k % every_b == 3)] = BEARING
    fixed_p = set(int(i) for i in g["fixed_poses"]); fixed_l = set(int(i) for i in g["fixed_landmarks"])
    cnt = np.bincount(pl_l, minlength=len(g["lm_est"]))
    cone = next(l for l in range(len(cnt)) if cnt[l] >= 2 and l not in fixed_l)
    model[(pl_l == cone) & (model == 0)] = RANGE_BEARING
    pose = next(int(p) for p in np.unique(pl_p)[2:] if int(p) not in fixed_p)
    on_pose = np.flatnonzero(pl_p == pose)
    model[on_pose[model[on_pose] == 0]] = RANGE_BEARING
    for e in np.flatnonzero(np.isin(pl_l, sorted(fixed_l)))[:1]:
        model[e] = RANGE_BEARING
    for e in np.flatnonzero(np.isin(pl_p, sorted(fixed_p)))[:1]:
        model[e] = BEARING if model[e] == 0 else model[e]
    idx = np.flatnonzero(model > 0)
    r = np.hypot(z[idx, 0], z[idx, 1]); beta = np.arctan2(z[idx, 1], z[idx, 0])
    Om = np.zeros((len(idx), 2, 2))
    Om[:, 0, 0] = W[idx, 0, 0]; Om[:, 0, 1] = Om[:, 1, 0] = W[idx, 0, 1] * r; Om[:, 1, 1] = W[idx, 1, 1] * r * r
    b_only = model[idx] == BEARING
    Om[b_only, 0, 0] = 0.0; Om[b_only, 0, 1] = 0.0; Om[b_only, 1, 0] = 0.0
    zz = np.stack([np.where(b_only, 0.0, r), beta], axis=1)
    return dict(idx=idx.astype(np.int64), model=model[idx].astype(np.int32), z=zz, W=Om, all_polar_pose=pose, all_polar_cone=cone)


def empty_set():
    return dict(idx=np.zeros(0, dtype=np.int64), model=np.zeros(0, dtype=np.int32), z=np.zeros((0, 2)), W=np.zeros((0, 2, 2)))


def subset(polar, keep):
    keep = np.asarray(keep)
    return dict(idx=polar["idx"][keep], model=polar["model"][keep], z=polar["z"][keep], W=polar["W"][keep])


def add_edges(G, g, polar, first=0, last=None, ids_pose=None, ids_lm=None):
    """the observation edges [first, last) of the graph dict into a handle in index order: runs of Cartesian edges through the bulk call,
    polar edges through the call of their model (single and bulk forms alternate)"""
    E = len(g["pl_p"]); last = E if last is None else last
    model = np.zeros(E, dtype=np.int32); model[polar["idx"]] = polar["model"]
    at = {int(e): t for t, e in enumerate(polar["idx"])}
    pl_p = np.asarray(g["pl_p"]); pl_l = np.asarray(g["pl_l"])
    if ids_pose is not None: pl_p = np.asarray(ids_pose)[pl_p]
    if ids_lm is not None: pl_l = np.asarray(ids_lm)[pl_l]
    k = first; run = 0
    while k < last:
        j = k
        while j < last and model[j] == model[k]:
            j += 1
        if model[k] == 0:
            G.add_observation_edges(pl_p[k:j], pl_l[k:j], np.asarray(g["pl_z"]).reshape(-1, 2)[k:j], np.asarray(g["pl_info"]).reshape(-1, 4)[k:j])
        else:
            t = [at[e] for e in range(k, j)]
            if model[k] == RANGE_BEARING:
                if run % 2 == 0 and j - k == 1:
                    G.add_range_bearing_edge(pl_p[k], pl_l[k], polar["z"][t[0]], polar["W"][t[0]])
                else:
                    G.add_range_bearing_edges(pl_p[k:j], pl_l[k:j], polar["z"][t], polar["W"][t].reshape(-1, 4))
            else:
                if run % 2 == 0 and j - k == 1:
                    G.add_bearing_edge(pl_p[k], pl_l[k], polar["z"][t[0], 1], polar["W"][t[0], 1, 1])
                else:
                    G.add_bearing_edges(pl_p[k:j], pl_l[k:j], polar["z"][t, 1], polar["W"][t, 1, 1])
            run += 1
        k = j


def load(G, g, polar):
    """load_bench_graph with the polar edges in place of their Cartesian ones"""
    N, M = len(g["pose_est"]), len(g["lm_est"])
    G.add_poses(np.arange(N), g["pose_est"]); G.add_landmarks(np.arange(M), g["lm_est"])
    G.add_odometry_edges(g["pp_i"], g["pp_j"], g["pp_z"], g["pp_info"])
    add_edges(G, g, polar)
    for i in g["fixed_poses"]:
        G.set_fixed_pose(int(i))
    for l in g["fixed_landmarks"]:
        G.set_fixed_landmark(int(l))
    return G


def carriers(g, polar, P=None, L=None):
    """the graph dict with what the handle's host graph holds for a polar edge: z = (0, 0), information 0"""
    out = dict(g)
    z = np.array(g["pl_z"], dtype=np.float64, copy=True).reshape(-1, 2); W = np.array(g["pl_info"], dtype=np.float64, copy=True).reshape(-1, 4)
    z[polar["idx"]] = 0.0; W[polar["idx"]] = 0.0
    out["pl_z"] = z; out["pl_info"] = W
    if P is not None: out["pose_est"] = np.array(P, dtype=np.float64, copy=True)
    if L is not None: out["lm_est"] = np.array(L, dtype=np.float64, copy=True)
    return out


def frame_points(g, polar, P, L):
    """d = x_p^-1 * l of the polar edges, in the oracle's operation order (robust_ref.errors_pl with z = 0)"""
    sub = dict(pl_p=np.asarray(g["pl_p"])[polar["idx"]], pl_l=np.asarray(g["pl_l"])[polar["idx"]], pl_z=np.zeros((len(polar["idx"]), 2)))
    return rr.errors_pl(sub, P, L)


def jd_of(d):
    """(Jd [n, 2, 2], Jd^-1 [n, 2, 2], r, valid); rows of invalid (r == 0) edges are zero"""
    dx, dy = d[:, 0], d[:, 1]; r2 = dx * dx + dy * dy; ok = r2 > 0
    r = np.sqrt(r2); rs = np.where(ok, r, 1.0); r2s = np.where(ok, r2, 1.0)
    Jd = np.stack([np.stack([dx / rs, dy / rs], 1), np.stack([-dy / r2s, dx / r2s], 1)], 1)
    Ji = np.stack([np.stack([dx / rs, -dy], 1), np.stack([dy / rs, dx], 1)], 1)
    Jd[~ok] = 0.0; Ji[~ok] = 0.0
    return Jd, Ji, r, ok


def terms(g, polar, P, L):
    """plain numpy, per polar edge: dict(e [n, 2], A [n, 2, 3], B [n, 2, 2], s [n], ok [n], Jd, Ji, d)"""
    P = np.asarray(P, dtype=np.float64); L = np.asarray(L, dtype=np.float64)
    d = frame_points(g, polar, P, L)
    Jd, Ji, r, ok = jd_of(d)
    beta = np.arctan2(d[:, 1], d[:, 0])
    e = np.stack([r - polar["z"][:, 0], rr.normalize_theta(beta - polar["z"][:, 1])], 1)
    e[~ok] = 0.0
    th = P[np.asarray(g["pl_p"])[polar["idx"]], 2]; c, s = np.cos(th), np.sin(th)
    Rt = np.stack([np.stack([c, s], 1), np.stack([-s, c], 1)], 1)
    B = np.einsum("nij,njk->nik", Jd, Rt)
    A = np.concatenate([-B, np.stack([np.zeros(len(d)), np.where(ok, -1.0, 0.0)], 1)[:, :, None]], axis=2)
    sq = np.einsum("ni,nij,nj->n", e, polar["W"], e)
    return dict(e=e, A=A, B=B, s=sq, ok=ok, Jd=Jd, Ji=Ji, d=d)


def contributions(g, polar, P, L, kernels=None, off=()):
    """what the polar edges add, plain numpy: dict(Hpp_diag [N, 9], Hll_diag [M, 4], Hpl [Epl, 6], b_pose [N, 3], b_lm [M, 2], chi2),
    summed in insertion order; fixed endpoints stay out of H, an edge between two fixed vertices out of chi2; off: inactive edges"""
    kernel = (kernels or {}).get("observation", rr.NONE)
    t = terms(g, polar, P, L)
    N, M, Epl = len(P), len(L), len(g["pl_p"])
    fp = np.zeros(N, dtype=bool); fp[np.asarray(g["fixed_poses"], dtype=np.int64)] = True
    fl = np.zeros(M, dtype=bool); fl[np.asarray(g["fixed_landmarks"], dtype=np.int64)] = True
    out = dict(Hpp_diag=np.zeros((N, 9)), Hll_diag=np.zeros((M, 4)), Hpl=np.zeros((Epl, 6)), b_pose=np.zeros((N, 3)), b_lm=np.zeros((M, 2)), chi2=0.0)
    w = rr.weight(kernel, t["s"]); rho = rr.rho(kernel, t["s"]); off = set(int(k) for k in off)
    for n, k in enumerate(polar["idx"]):
        if not t["ok"][n] or int(k) in off:
            continue
        p, l = int(g["pl_p"][k]), int(g["pl_l"][k]); A, B, W, e = t["A"][n], t["B"][n], w[n] * polar["W"][n], t["e"][n]
        if not (fp[p] and fl[l]): out["chi2"] += float(rho[n])
        if not fp[p]: out["Hpp_diag"][p] += (A.T @ W @ A).reshape(9); out["b_pose"][p] -= A.T @ W @ e
        if not fl[l]: out["Hll_diag"][l] += (B.T @ W @ B).reshape(4); out["b_lm"][l] -= B.T @ W @ e
        if not fp[p] and not fl[l]: out["Hpl"][k] = (A.T @ W @ B).reshape(6)
    return out


def edge_s(g, polar, P, L):
    """s = e^T Omega e of every observation edge, insertion order: the polar edges' own, the Cartesian edges' as robust_ref has them"""
    s = rr.edge_s(g, P, L)[1].copy()
    s[polar["idx"]] = terms(g, polar, P, L)["s"]
    return s


def cartesianised(g, polar, P, L, off=()):
    """the graph dict at (P, L) with every polar edge rewritten as the Cartesian edge that is equivalent there; off: inactive edges
    (information 0, of either kind)"""
    P = np.array(P, dtype=np.float64, copy=True); L = np.array(L, dtype=np.float64, copy=True)
    out = dict(g); out["pose_est"] = P; out["lm_est"] = L
    z = np.array(g["pl_z"], dtype=np.float64, copy=True).reshape(-1, 2); W = np.array(g["pl_info"], dtype=np.float64, copy=True).reshape(-1, 4)
    if len(polar["idx"]):
        t = terms(g, polar, P, L)
        e = t["e"].copy(); e[polar["model"] == BEARING, 0] = 0.0
        z[polar["idx"]] = t["d"] - np.einsum("nij,nj->ni", t["Ji"], e)
        Wc = np.einsum("nji,njk,nkl->nil", t["Jd"], polar["W"], t["Jd"])
        W[polar["idx"]] = ((Wc + np.transpose(Wc, (0, 2, 1))) / 2).reshape(-1, 4)
    for k in off:
        W[int(k)] = 0.0
    out["pl_z"] = z; out["pl_info"] = W
    return out


def chi2_at(po, g, polar, P, L, kernels=None, off=()):
    from conftest import make_oracle_graph
    gc = cartesianised(g, polar, P, L, off)
    return rr.robust_chi2(gc, P, L, kernels) if kernels else make_oracle_graph(po, gc).chi2()


def oracle_at(po, g, polar, P, L, kernels=None, off=()):
    """the oracle graph whose linearisation at (P, L) is the polar graph's (re-weighted when kernels are set)"""
    from conftest import make_oracle_graph
    gc = cartesianised(g, polar, P, L, off)
    return make_oracle_graph(po, rr.reweighted(gc, P, L, kernels) if kernels else gc)


def gauss_newton(po, g, polar, iterations, P=None, L=None, kernels=None, off=()):
    """Gauss-Newton with the oracle, re-cartesianised at every iterate.  Returns (P, L, chi[it] at the linearisation points, the last
    increment (dpose, dlm), chi2 at the end)"""
    P = np.array(g["pose_est"] if P is None else P, dtype=np.float64, copy=True); L = np.array(g["lm_est"] if L is None else L, dtype=np.float64, copy=True)
    chi = []; delta = None
    for _ in range(iterations):
        chi.append(chi2_at(po, g, polar, P, L, kernels, off))
        og = oracle_at(po, g, polar, P, L, kernels, off)
        done, _, _ = og.optimize(1, ordering=1); assert done == 1
        P, L = og.poses(), og.landmarks(); delta = og.delta()
    return P, L, np.array(chi), delta, chi2_at(po, g, polar, P, L, kernels, off)


# ---------------------------------------------------------------- Levenberg-Marquardt: lm_ref.run restated over this system_at
def system_at(po, g, polar, P, L, kernels):
    og = oracle_at(po, g, polar, P, L, kernels)
    chi = chi2_at(po, g, polar, P, L, kernels)
    n, colptr, rowind, values, b = og.build_system()
    return og, n, colptr, rowind, values, b, chi


def lm_trial(po, g, polar, P, L, lam, kernels=None):
    kernels = kernels or {}
    og, n, colptr, rowind, values, b, chi_old = system_at(po, g, polar, P, L, kernels)
    dp = lm_ref.diag_positions(n, colptr, rowind)
    max_diag = float(np.abs(values[dp]).max())
    v = values.copy(); v[dp] += lam
    x = lm_ref._solve(po, n, colptr, rowind, v, b)
    og.apply_update(x)
    Pt, Lt = og.poses(), og.landmarks(); dpose, dlm = og.delta()
    chi_new = chi2_at(po, g, polar, Pt, Lt, kernels)
    scale = float(np.sum(x * (lam * x + b))) + 1e-3
    return dict(P=Pt, L=Lt, dpose=dpose, dlm=dlm, chi_old=chi_old, chi_new=chi_new, scale=scale, rho=(chi_old - chi_new) / scale, max_diag=max_diag)


def lm_run(po, g, polar, iterations, kernels=None, initial_lambda=0.0, tau=1e-5, max_trials=10, poses=None, lms=None):
    """lm_ref.run's loop (same rule, same log) with the system and chi2 of the polar graph"""
    kernels = kernels or {}
    P = np.array(g["pose_est"] if poses is None else poses, dtype=np.float64, copy=True)
    L = np.array(g["lm_est"] if lms is None else lms, dtype=np.float64, copy=True)
    lam = float(initial_lambda) if initial_lambda > 0 else None
    nu = 2.0; log = []; n_trials = []; chi_it = []; lam_it = []; accepted = rejected = 0; terminated = False; lam0 = lam
    chi_final = None
    for it in range(iterations):
        q = 0; ok = False
        while q < max_trials:
            if lam is None:
                _, n, colptr, rowind, values, _, _ = system_at(po, g, polar, P, L, kernels)
                lam = tau * float(np.abs(values[lm_ref.diag_positions(n, colptr, rowind)]).max()); lam0 = lam
            t = lm_trial(po, g, polar, P, L, lam, kernels)
            good = t["rho"] > 0 and np.isfinite(t["chi_new"])
            margin = abs(t["chi_old"] - t["chi_new"]) / t["chi_old"]
            log.append(dict(iteration=it, lam=lam, chi_old=t["chi_old"], chi_new=t["chi_new"], rho=t["rho"], accepted=good, margin=margin,
                            dpose=t["dpose"], dlm=t["dlm"]))
            if q == 0:
                chi_it.append(t["chi_old"]); lam_it.append(lam)
            lam_it[-1] = lam
            if chi_final is None:
                chi_final = t["chi_old"]
            q += 1
            if good:
                a = 2.0 * t["rho"] - 1.0
                alpha = min(1.0 - a * a * a, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha); nu = 2.0
                P, L = t["P"], t["L"]; chi_final = t["chi_new"]; accepted += 1; ok = True
                break
            lam *= nu; nu *= 2.0; rejected += 1
        n_trials.append(q)
        if not ok:
            terminated = True
            break
    return dict(trials=log, n_trials=np.array(n_trials, dtype=np.int32), chi2=np.array(chi_it), lam=np.array(lam_it), accepted=accepted,
                rejected=rejected, terminated=terminated, lambda_initial=lam0, lambda_final=lam, chi2_final=chi_final, P=P, L=L,
                min_margin=min([t["margin"] for t in log]) if log else np.inf)
