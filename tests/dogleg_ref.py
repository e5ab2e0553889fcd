"""Checker of gs_optimize_dogleg (numpy + the CPU oracle): g2o's OptimizationAlgorithmDogleg rule, restated from g2o's published text
(not pinned against a g2o build), on OracleGraph; modelled on lm_ref.py.

State: the trust radius delta.  Per iteration at the accepted estimates x: chi_old = chi2(x); H, b = the oracle's scalar upper CCS at x;
alpha = b.b / b.Hb (0 unless b.Hb is finite and > 0), h_sd = alpha b; h_gn = the solve of lm_ref._solve; trials: |h_gn| < delta: h_gn (GN);
else |h_sd| > delta: (delta / |h_sd|) h_sd (SD); else h_sd + beta (h_gn - h_sd) (DL, beta as in include/graphslam.h); gain = -h.Hh + 2 b.h
(|gain| < 1e-12: 1e-12); x_try = x [+] h (the oracle's update); rho = (chi_old - chi_new) / gain; accept if rho > 0 and chi_new is
finite, else put x back; rho > 0.75: delta = max(delta, 3 |h|); rho < 0.25: delta /= 2.  All trials of an iteration rejected: terminate.

Model(...) is the graph the rule runs on: robust kernels (robust_ref), a polar set (polar_ref: re-cartesianised at every point), priors
(prior_ref.augment) and inactive observation edges, alone or together.

run(...) returns the full trial log.  Per trial: kind, delta, |h_gn|, |h_sd|, rho, margin = |chi_old - chi_new| / chi_old, and how far
the two branch comparisons were from a tie (relative).  conditions(r) asserts what makes a GPU / CPU comparison of decisions meaningful."""
import numpy as np

import lm_ref
import polar_ref as plr
import prior_ref as pr
import robust_ref as rr
from conftest import make_oracle_graph

GN, SD, DL = 0, 1, 2
KINDS = ("GN", "SD", "DL")
MIN_MARGIN = 1e-3            # |chi_old - chi_new| / chi_old of every trial
MIN_RHO_GAP = 1e-2           # distance of every rho from 0, 0.25 and 0.75
MIN_BRANCH_GAP = 1e-3        # relative distance of |h_gn| and |h_sd| from delta where they were compared


class Model:
    def __init__(self, po, g, kernels=None, polar=None, pri=None, off=()):
        self.po, self.g, self.kernels, self.polar, self.pri, self.off = po, g, kernels or {}, polar, pri, tuple(off)
        self.N = len(g["pose_est"])

    def graph_at(self, P, L):
        if self.polar is not None or self.off:
            return plr.cartesianised(self.g, self.polar if self.polar is not None else plr.empty_set(), P, L, self.off)
        return dict(self.g, pose_est=np.array(P, dtype=np.float64, copy=True), lm_est=np.array(L, dtype=np.float64, copy=True))

    def chi2(self, P, L):
        gc = self.graph_at(P, L)
        chi = rr.robust_chi2(gc, P, L, self.kernels) if self.kernels else make_oracle_graph(self.po, gc).chi2()
        if self.pri is not None:
            chi += pr.contributions(self.g, self.pri, P, L)[4]
        return float(chi)

    def system(self, P, L):
        """(oracle graph, n, colptr, rowind, values, b) at (P, L)"""
        gc = self.graph_at(P, L)
        if self.kernels:
            gc = rr.reweighted(gc, P, L, self.kernels)
        if self.pri is not None:
            gc = pr.augment(gc, self.pri)
        og = make_oracle_graph(self.po, gc)
        return (og,) + tuple(og.build_system())

    def step(self, og, x):
        """x_try = x [+] h: (P, L, dpose, dlm)"""
        og.apply_update(x)
        dp, dl = og.delta()
        return og.poses()[:self.N], og.landmarks(), dp[:self.N], dl


def sym_mul(n, colptr, rowind, values, x):
    """H x with H given as its scalar upper CCS"""
    cols = np.repeat(np.arange(n), np.diff(colptr)); off = rowind != cols
    return np.bincount(rowind, values * x[cols], minlength=n) + np.bincount(cols[off], values[off] * x[rowind[off]], minlength=n)


def alpha_of(b, Hb):
    bHb = float(b @ Hb)
    return float(b @ b) / bHb if np.isfinite(bHb) and bHb > 0 else 0.0


def blend(h_gn, h_sd, delta):
    """(h_dl, kind, |h_gn|, |h_sd|, gaps): gaps = relative distances of the comparisons made from a tie"""
    gn, sd = float(np.linalg.norm(h_gn)), float(np.linalg.norm(h_sd))
    gaps = [abs(gn - delta) / delta]
    if gn < delta:
        return h_gn.copy(), GN, gn, sd, gaps
    gaps.append(abs(sd - delta) / delta)
    if sd > delta:
        return (delta / sd) * h_sd, SD, gn, sd, gaps
    a = h_gn - h_sd; c = float(h_sd @ a); q = float(a @ a); m = delta * delta - sd * sd
    disc = np.sqrt(c * c + q * m)
    beta = 0.0 if q == 0 else ((-c + disc) / q if c <= 0 else m / (c + disc))
    return h_sd + beta * a, DL, gn, sd, gaps


class Point:
    """the linearisation at an accepted point: shared by the retrials of an iteration (they are bit-identical)"""
    def __init__(self, model, P, L):
        self.P, self.L = P, L
        self.og, self.n, self.colptr, self.rowind, self.values, self.b = model.system(P, L)
        self.chi = model.chi2(P, L)
        self.h_sd = alpha_of(self.b, sym_mul(self.n, self.colptr, self.rowind, self.values, self.b)) * self.b
        self.h_gn = lm_ref._solve(model.po, self.n, self.colptr, self.rowind, self.values, self.b)


def trial(model, pt, delta):
    h, kind, gn, sd, gaps = blend(pt.h_gn, pt.h_sd, delta)
    gain = float(-(h @ sym_mul(pt.n, pt.colptr, pt.rowind, pt.values, h)) + 2.0 * (pt.b @ h))
    if abs(gain) < 1e-12:
        gain = 1e-12
    og = model.system(pt.P, pt.L)[0]                        # a fresh graph at x: the oracle's update moves its estimates
    P, L, dpose, dlm = model.step(og, h)
    chi_new = model.chi2(P, L)
    rho = (pt.chi - chi_new) / gain
    hn = float(np.linalg.norm(h))
    nxt = max(delta, 3.0 * hn) if rho > 0.75 else (0.5 * delta if rho < 0.25 else delta)
    return dict(kind=kind, delta=delta, gn=gn, sd=sd, gaps=gaps, gain=gain, rho=rho, chi_old=pt.chi, chi_new=chi_new, hdl=hn, delta_next=nxt,
                accepted=bool(rho > 0 and np.isfinite(chi_new)), margin=abs(pt.chi - chi_new) / pt.chi, P=P, L=L, dpose=dpose, dlm=dlm)


def first_norms(model, P=None, L=None):
    """(|h_gn|, |h_sd|) at the start: what a test sizes initial_delta with to reach a given kind"""
    pt = Point(model, np.array(model.g["pose_est"] if P is None else P, dtype=np.float64), np.array(model.g["lm_est"] if L is None else L, dtype=np.float64))
    return float(np.linalg.norm(pt.h_gn)), float(np.linalg.norm(pt.h_sd))


def run(model, iterations, initial_delta=1e4, max_trials=100, poses=None, lms=None):
    """dict(trials=[...], n_trials, chi2, delta, kind (per iteration: of the accepted or last trial), accepted, rejected, terminated,
    delta_final, chi2_final, P, L)"""
    P = np.array(model.g["pose_est"] if poses is None else poses, dtype=np.float64, copy=True)
    L = np.array(model.g["lm_est"] if lms is None else lms, dtype=np.float64, copy=True)
    delta = float(initial_delta); log = []; n_trials = []; chi_it = []; delta_it = []; kind_it = []
    accepted = rejected = 0; terminated = False; chi_final = None
    for it in range(iterations):
        pt = Point(model, P, L)
        if chi_final is None:
            chi_final = pt.chi
        chi_it.append(pt.chi); delta_it.append(delta); kind_it.append(-1)
        q = 0; ok = False
        while q < max_trials:
            t = trial(model, pt, delta); t["iteration"] = it
            log.append(t); delta_it[-1] = delta; kind_it[-1] = t["kind"]; q += 1
            delta = t["delta_next"]
            if t["accepted"]:
                P, L = t["P"], t["L"]; chi_final = t["chi_new"]; accepted += 1; ok = True
                break
            rejected += 1
        n_trials.append(q)
        if not ok:
            terminated = True
            break
    return dict(trials=log, n_trials=np.array(n_trials, dtype=np.int32), chi2=np.array(chi_it), delta=np.array(delta_it), kind=np.array(kind_it, dtype=np.int32),
                accepted=accepted, rejected=rejected, terminated=terminated, delta_final=delta, chi2_final=chi_final, P=P, L=L)


def rho_gap(rho):
    return min(abs(rho), abs(rho - 0.25), abs(rho - 0.75))


def figures(r):
    """(smallest margin, smallest rho gap, smallest branch gap) over the trials"""
    T = r["trials"]
    return min(t["margin"] for t in T), min(rho_gap(t["rho"]) for t in T), min(min(t["gaps"]) for t in T)


def conditions(r):
    """every trial far enough from a tie in its verdict, its delta update and its choice of step"""
    for t in r["trials"]:
        assert t["margin"] >= MIN_MARGIN and rho_gap(t["rho"]) >= MIN_RHO_GAP and min(t["gaps"]) >= MIN_BRANCH_GAP, describe(dict(trials=[t]))


def describe(r):
    """one line per trial, for the tests' printed record"""
    return "\n".join("  it %d %s delta %.6g |h_gn| %.6g |h_sd| %.6g chi_old %.10g chi_new %.10g rho %+.4f %s margin %.3g" % (
        t.get("iteration", 0), KINDS[t["kind"]], t["delta"], t["gn"], t["sd"], t["chi_old"], t["chi_new"], t["rho"],
        "accept" if t["accepted"] else "REJECT", t["margin"]) for t in r["trials"])
