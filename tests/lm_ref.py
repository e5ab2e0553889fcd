"""Checker of gs_optimize_lm (numpy + the CPU oracle): g2o's OptimizationAlgorithmLevenberg rule, restated from g2o's published
text (not pinned against a g2o build), on OracleGraph.

Per iteration at the accepted estimates x: chi_old = chi2(x); H, b = the oracle's scalar upper CCS at x (with robust kernels: of
robust_ref.reweighted(...), chi2 = robust_ref.robust_chi2); first iteration without a lambda: lambda = tau * max |H_jj|; trials:
solve (H + lambda I) D = b with the reference's Eigen LDLT (oracle/_ref; a dense numpy solve when that is absent), x_try = x [+] D
(the oracle's update), chi_new = chi2(x_try), scale = sum D (lambda D + b) + 1e-3, rho = (chi_old - chi_new) / scale; accept if
rho > 0 and chi_new is finite: lambda *= max(1/3, min(1 - (2 rho - 1)^3, 2/3)), nu = 2; else put x back, lambda *= nu, nu *= 2.
All trials of an iteration rejected: terminate.

run(...) returns the full trial log; margin = |chi_old - chi_new| / chi_old says how far a trial's verdict is from rounding noise
(a GPU / CPU comparison of accept / reject decisions needs margin >= MIN_MARGIN on every trial)."""
import numpy as np

import robust_ref as rr
from conftest import make_oracle_graph

MIN_MARGIN = 1e-3


def _solve(po, n, colptr, rowind, values, b):
    if po.ref_eigen() is not None:
        return po.EigenSolver(0).solve(n, colptr, rowind, values, b)
    A = np.zeros((n, n))
    for j in range(n):
        for k in range(colptr[j], colptr[j + 1]):
            A[rowind[k], j] = values[k]; A[j, rowind[k]] = values[k]
    return np.linalg.solve(A, b)


def diag_positions(n, colptr, rowind):
    """index into `values` of every diagonal entry of the upper CCS"""
    pos = np.zeros(n, dtype=np.int64)
    for j in range(n):
        k = np.flatnonzero(rowind[colptr[j]:colptr[j + 1]] == j)
        assert len(k) == 1
        pos[j] = colptr[j] + k[0]
    return pos


def system_at(po, g, P, L, kernels):
    """(oracle graph at (P, L) — re-weighted when kernels are set —, n, colptr, rowind, values, b, chi2 at (P, L))"""
    if kernels:
        og = make_oracle_graph(po, rr.reweighted(g, P, L, kernels)); chi = rr.robust_chi2(g, P, L, kernels)
    else:
        gg = dict(g); gg["pose_est"] = np.asarray(P, dtype=np.float64); gg["lm_est"] = np.asarray(L, dtype=np.float64)
        og = make_oracle_graph(po, gg); chi = og.chi2()
    n, colptr, rowind, values, b = og.build_system()
    return og, n, colptr, rowind, values, b, chi


def chi2_at(po, g, og, P, L, kernels):
    return rr.robust_chi2(g, P, L, kernels) if kernels else og.chi2()


def trial(po, g, P, L, lam, kernels=None):
    """one damped step from (P, L): dict(P, L = x_try, dpose, dlm, chi_old, chi_new, scale, rho, max_diag)"""
    kernels = kernels or {}
    og, n, colptr, rowind, values, b, chi_old = system_at(po, g, P, L, kernels)
    dp = diag_positions(n, colptr, rowind)
    max_diag = float(np.abs(values[dp]).max())
    v = values.copy(); v[dp] += lam
    x = _solve(po, n, colptr, rowind, v, b)
    og.apply_update(x)
    Pt, Lt = og.poses(), og.landmarks(); dpose, dlm = og.delta()
    chi_new = chi2_at(po, g, og, Pt, Lt, kernels)
    scale = float(np.sum(x * (lam * x + b))) + 1e-3
    return dict(P=Pt, L=Lt, dpose=dpose, dlm=dlm, chi_old=chi_old, chi_new=chi_new, scale=scale, rho=(chi_old - chi_new) / scale, max_diag=max_diag)


def max_diag(po, g, P, L, kernels=None):
    _, n, colptr, rowind, values, _, _ = system_at(po, g, P, L, kernels or {})
    return float(np.abs(values[diag_positions(n, colptr, rowind)]).max())


def run(po, g, iterations, kernels=None, initial_lambda=0.0, tau=1e-5, max_trials=10, poses=None, lms=None, force_reject=()):
    """force_reject: trial ordinals (0-based, over the call) rejected whatever their rho — a zero pivot in that trial's
    factorisation (g2o: rho = -1).  Returns dict(trials=[...], n_trials, chi2, lam (per iteration), accepted, rejected, terminated,
    lambda_initial, lambda_final, chi2_final, P, L, min_margin)."""
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
                lam = tau * max_diag(po, g, P, L, kernels); lam0 = lam
            t = trial(po, g, P, L, lam, kernels)
            forced = len(log) in force_reject
            good = (not forced) and t["rho"] > 0 and np.isfinite(t["chi_new"])
            margin = abs(t["chi_old"] - t["chi_new"]) / t["chi_old"]
            log.append(dict(iteration=it, lam=lam, chi_old=t["chi_old"], chi_new=t["chi_new"], rho=-1.0 if forced else t["rho"], accepted=good,
                            margin=np.inf if forced else margin, dpose=t["dpose"], dlm=t["dlm"]))
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


def describe(r):
    """one line per trial, for the tests' printed record"""
    return "\n".join("  it %d lambda %.6e chi_old %.10g chi_new %.10g rho %+.4f %s margin %.3g" % (
        t["iteration"], t["lam"], t["chi_old"], t["chi_new"], t["rho"], "accept" if t["accepted"] else "REJECT", t["margin"]) for t in r["trials"])
