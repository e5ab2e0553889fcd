"""The step control of gs_optimize_dogleg and gs_optimize_lm redone exactly, with a counted rounding bound on every result (TEST-ONLY).

Written from the rules as include/graphslam.h, csrc/gs_dogleg.hpp and csrc/gs_lm.hpp state them, not from the kernels:
    dogleg   alpha = b.b / b.Hb (0 unless b.Hb is finite and > 0), h_sd = alpha b, a = h_gn - h_sd, gg = |h_gn|^2, ss = |h_sd|^2, cc = h_sd.a,
             qq = a.a; sqrt(gg) < delta: GN, else sqrt(ss) > delta: SD, h = (delta / |h_sd|) h_sd, else DL, h = h_sd + beta a with
             m = delta^2 - ss, beta = (-cc + sqrt(cc^2 + qq m)) / qq (cc <= 0) or m / (cc + sqrt(cc^2 + qq m)); gain = -h.Hh + 2 b.h
             (|gain| < 1e-12: 1e-12); rho = (chi_old - chi_new) / gain; rho > 0.75: delta = max(delta, 3 |h|), rho < 0.25: delta / 2
    LM       scale = sum dx (lambda dx + b) + 1e-3; rho = (chi_old - chi_new) / scale; accepted: lambda * max(1/3, min(1 - (2 rho - 1)^3, 2/3)),
             rejected: 2 lambda (the first rejection); lambda_0 = tau max |H_jj| over the free scalars
Inputs are fp64 numbers taken exactly: H as the six block arrays of an export with the graph dict (hmul_ref.py's conventions: vertex
order, rows and columns of fixed vertices zero) or as an upper CCS over the free scalars, b, h_gn or the LM increment, delta or lambda,
chi_old and chi_new.  Sums of products of fp64 numbers are formed without error (TwoProd, then math.fsum, three times for 159 bits);
everything behind them is mpmath at 60 digits.  Since h_sd = alpha b and h = s b + t h_gn for two scalars s and t, every reduction of the
rule is a combination of six such sums: b.b, b.Hb, b.h_gn, h_gn.h_gn, b.H h_gn, h_gn.H h_gn.

Every result is a Val(value, bound): |device - value| <= bound for ANY fp64 evaluation of the rule, by the standard model — one
u = 2^-53 of the result per + - * / sqrt; a sum of n terms in any grouping (lanes, waves, workgroups, partials) (n - 1) u of the sum of
the absolute values; an input that carries a bound passes it on to first order; FMA contraction only removes roundings.  n = the free
scalars.  The counts (E_x: the bound of x; A(x.y) = sum |x_i| |y_i|):
    Hv_i     the device product: hmul_ref's 2 (n_i + 2) u (|H| |v|)_i, n_i the products of row i                              = eH_i
    b.b      product 1, sum n - 1                                                   E = n u b.b
    b.Hb     Hb_i eH_i, product 1, sum n - 1                                        E = sum |b_i| eH_i + n u A(b.Hb)
    alpha    b.b, b.Hb, division 1                                                  E = alpha (E_bb / bb + E_bHb / bHb + u)
    h_sd_i   alpha, product 1                                                       e_s = |b_i| E_alpha + u |h_sd_i|
    a_i      h_sd_i, subtraction 1                                                  e_a = e_s + u |a_i|
    gg       product 1, sum n - 1                                                   E = n u gg
    ss       h_sd twice, product 1, sum n - 1                                       E = sum 2 |h_sd_i| e_s + n u ss
    cc       h_sd, a, product 1, sum n - 1                                          E = sum (|a_i| e_s + |h_sd_i| e_a) + n u A(h_sd.a)
    qq       a twice, product 1, sum n - 1                                          E = sum 2 |a_i| e_a + n u qq
    |h_gn|, |h_sd|   sqrt 1                                                         E = E_gg / (2 |h_gn|) + u |h_gn|
    SD scale |h_sd|, division 1                                                     E = scale (E_sd / |h_sd| + u)
    SD h_i   scale, h_sd_i, product 1                                               e_h = |h_sd_i| E_scale + scale e_s + u |h_i|
    m        delta^2 1, ss, subtraction 1                                           E = u delta^2 + E_ss + u |m|
    r = cc^2 + qq m   cc twice, product 1, qq, m, product 1, addition 1             E = 2 |cc| E_cc + u cc^2 + |m| E_qq + qq E_m + u |qq m| + u r
    disc     r, sqrt 1                                                              E = E_r / (2 disc) + u disc
    beta     cc <= 0: cc, disc, addition 1, qq, division 1                          E = (E_cc + E_disc + u |num|) / qq + |beta| E_qq / qq + u |beta|
             cc > 0: m, cc, disc, addition 1, division 1                            E = E_m / den + |beta| (E_cc + E_disc + u den) / den + u |beta|
             (where the sign of cc is within E_cc of 0 the larger of the two)
    DL h_i   h_sd_i, beta, a_i, product 1, addition 1                               e_h = e_s + |a_i| E_beta + |beta| e_a + u |beta a_i| + u |h_i|
    hh       h twice, product 1, sum n - 1                                          E = sum 2 |h_i| e_h + n u hh
    h.Hh     (Hh)_i eH_i, h twice, product 1, sum n - 1                             E = sum |h_i| eH_i + 2 sum e_h |Hh_i| + n u A(h.Hh)
    b.h      h, product 1, sum n - 1                                                E = sum |b_i| e_h + n u A(b.h)
    gain     h.Hh, b.h doubled (exact), addition 1                                  E = E_hHh + 2 E_bh + u |gain|
    rho      chi_old - chi_new 1 (the handle's own two numbers), gain, division 1   E = |rho| (2 u + E_gain / |gain|)
    3 |h|    hh, sqrt 1, product 1                                                  E = 3 (E_hh / (2 |h|) + u |h|) + 3 u |h|
    LM scale per term lambda dx 1, + b 1, dx * 1, sum n - 1, + 1e-3 1               E = u sum (lambda dx^2 + 2 |dx| |lambda dx + b|) + (n - 1) u A + u |scale|
    LM rho   as above with scale                                                    E = |rho| (2 u + E_scale / |scale|)
    LM update   t = 2 rho - 1: 2 E_rho + u |t|; t^3 two products: 3 t^2 E_t + 2 u |t^3|; 1 - t^3: + u; lambda * factor: + u
    slots    a fused-path landmark's diagonal summed from k slots, lambda in the first: k u (H_jj + lambda) for the sum with lambda,
             (k - 1) u H_jj for the exported H_jj itself, u for fl(H_jj + lambda)  = 2 k u (H_jj + lambda); k <= the landmark's
             observation edges (one slot per wave tile that sees it), the slots of a diagonal scalar are all >= 0
A comparison is decided when the exact value is further from its threshold than its bound; only decided comparisons are judged."""
import math
from collections import namedtuple

import mpmath
import numpy as np

import exact_ref as xr
import hmul_ref as hr

MP = mpmath.mp.clone()
MP.dps = 60
mpf = MP.mpf
U = 2.0 ** -53
GN, SD, DL = 0, 1, 2
KINDS = ("GN", "SD", "DL")
Val = namedtuple("Val", "value bound")


def err_over_bound(got, val):
    """|got - value| / bound (0 / 0 = 0, x / 0 = inf)"""
    e = float(abs(mpf(float(got)) - val.value))
    return e / val.bound if val.bound > 0 else (0.0 if e == 0 else math.inf)


def xsum(terms):
    """the sum of fp64 numbers without error (to 159 bits)"""
    t = [float(v) for v in np.asarray(terms, dtype=np.float64).reshape(-1)]
    hi = math.fsum(t); lo = math.fsum(t + [-hi]); lo2 = math.fsum(t + [-hi, -lo])
    return mpf(hi) + mpf(lo) + mpf(lo2)


def xdot(u, v):
    p, e = xr.two_prod(np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64))
    return xsum(np.concatenate([p.reshape(-1), e.reshape(-1)]))


class System:
    """H as scalar triplets (both triangles) over n scalars, b, the products per row; free: the scalars that are not a fixed vertex's"""

    def __init__(self, rows, cols, vals, b, nprod, free, shape=None):
        o = np.argsort(rows, kind="stable")
        self.rows, self.cols, self.vals = rows[o], cols[o], np.asarray(vals, dtype=np.float64)[o]
        self.b = np.asarray(b, dtype=np.float64); self.n = len(self.b); self.nprod = np.asarray(nprod, dtype=np.float64)
        self.free = free; self.nf = int(free.sum()); self.shape = shape
        self.start = np.searchsorted(self.rows, np.arange(self.n + 1))

    @classmethod
    def from_blocks(cls, B, g):
        N, M = len(B["Hpp_diag"]), len(B["Hll_diag"])
        fp, fl = hr.masks(g, N, M)
        pi, pj = np.asarray(g["pp_i"], dtype=np.int64), np.asarray(g["pp_j"], dtype=np.int64)
        pp, pl = np.asarray(g["pl_p"], dtype=np.int64), np.asarray(g["pl_l"], dtype=np.int64)
        R, Cc, Vv = [], [], []

        def add(r0, wr, c0, wc, blocks, ok):
            for a in range(wr):
                for c in range(wc):
                    R.append(r0[ok] + a); Cc.append(c0[ok] + c); Vv.append(blocks[ok][:, a, c])
        ip, il = 3 * np.arange(N), 3 * N + 2 * np.arange(M)
        add(ip, 3, ip, 3, np.asarray(B["Hpp_diag"]).reshape(N, 3, 3), fp)
        add(il, 2, il, 2, np.asarray(B["Hll_diag"]).reshape(M, 2, 2), fl)
        O = np.asarray(B["Hpp_off"]).reshape(-1, 3, 3); W = np.asarray(B["Hpl"]).reshape(-1, 3, 2)
        ok = fp[pi] & fp[pj]; add(ip[pi], 3, ip[pj], 3, O, ok); add(ip[pj], 3, ip[pi], 3, O.transpose(0, 2, 1), ok)
        ok = fp[pp] & fl[pl]; add(ip[pp], 3, il[pl], 2, W, ok); add(il[pl], 2, ip[pp], 3, W.transpose(0, 2, 1), ok)
        b = np.concatenate([np.where(fp[:, None], B["b_pose"], 0.0).reshape(-1), np.where(fl[:, None], B["b_lm"], 0.0).reshape(-1)])
        n_pose = 3 + 3 * (np.bincount(pi, minlength=N) + np.bincount(pj, minlength=N)) + 2 * np.bincount(pp, minlength=N)
        n_lm = 2 + 3 * np.bincount(pl, minlength=M)
        return cls(np.concatenate(R), np.concatenate(Cc), np.concatenate(Vv), b, np.concatenate([np.repeat(n_pose, 3), np.repeat(n_lm, 2)]),
                   np.concatenate([np.repeat(fp, 3), np.repeat(fl, 2)]), shape=(N, M))

    @classmethod
    def from_ccs(cls, n, colptr, rowind, values, b):
        cols = np.repeat(np.arange(n), np.diff(colptr)); rows = np.asarray(rowind, dtype=np.int64); off = rows != cols
        R = np.concatenate([rows, cols[off]]); Cc = np.concatenate([cols, rows[off]]); Vv = np.concatenate([values, np.asarray(values)[off]])
        return cls(R, Cc, Vv, b, np.bincount(R, minlength=n), np.ones(n, dtype=bool))

    def pack(self, vp, vl):
        N, M = self.shape
        return np.where(self.free, np.concatenate([np.asarray(vp, dtype=np.float64).reshape(-1), np.asarray(vl, dtype=np.float64).reshape(-1)]), 0.0)

    def unpack(self, x):
        N, M = self.shape
        return x[:3 * N].reshape(N, 3), x[3 * N:].reshape(M, 2)

    def mul(self, v):
        """(H v per row, correctly rounded; (|H| |v|) per row)"""
        p, e = xr.two_prod(self.vals, v[self.cols]); y = np.zeros(self.n)
        for i in range(self.n):
            a, z = self.start[i], self.start[i + 1]
            if z > a:
                y[i] = math.fsum(p[a:z].tolist() + e[a:z].tolist())
        return y, np.bincount(self.rows, np.abs(self.vals) * np.abs(v[self.cols]), minlength=self.n)

    def quad(self, u, v):
        """u^T H v without error"""
        p, e = xr.two_prod(self.vals, v[self.cols]); w = u[self.rows]
        p1, e1 = xr.two_prod(p, w); p2, e2 = xr.two_prod(e, w)
        return xsum(np.concatenate([p1, e1, p2, e2]))

    def mul_bound(self, S):
        return 2.0 * (self.nprod + 2) * U * S


def _f(x):
    return float(x)


def gain_terms(S, hHh, bh, hh, h, e_h, delta, chi_old=None, chi_new=None):
    """gain, rho and delta_next with their bounds from the exact h.Hh, b.h, h.h of a step h (fp64 image `h`, per-scalar bound e_h)"""
    n = S.nf; Hh, SHh = S.mul(h); eHh = S.mul_bound(SHh); ah = np.abs(h); b = S.b
    E_hHh = float((ah * eHh).sum() + 2 * (e_h * np.abs(Hh)).sum() + n * U * (ah * np.abs(Hh)).sum())
    E_bh = float((np.abs(b) * e_h).sum() + n * U * (np.abs(b) * ah).sum())
    E_hh = float(2 * (ah * e_h).sum() + n * U * _f(hh))
    gain = -hHh + 2 * bh; E_gain = E_hHh + 2 * E_bh + U * abs(_f(gain))
    clamped = abs(gain) < mpf(1e-12)
    out = dict(Hh=(Hh, eHh), hHh=Val(hHh, E_hHh), bh=Val(bh, E_bh), hh=Val(hh, E_hh), gain=Val(mpf(1e-12) if clamped else gain, E_gain),
               clamp_decided=abs(abs(_f(gain)) - 1e-12) > E_gain)
    hn = MP.sqrt(hh); E_3h = (3 * (E_hh / (2 * _f(hn)) + U * _f(hn)) + 3 * U * _f(hn)) if hn > 0 else 0.0
    out["three_h"] = Val(3 * hn, E_3h)
    if chi_old is not None:
        g_ = out["gain"].value
        rho = (mpf(float(chi_old)) - mpf(float(chi_new))) / g_; E_rho = abs(_f(rho)) * (2 * U + E_gain / abs(_f(g_)))
        out["rho"] = Val(rho, E_rho)
        out["accept"] = bool(rho > 0 and math.isfinite(chi_new)); out["accept_decided"] = abs(_f(rho)) > E_rho
        out["rho_decided"] = min(abs(_f(rho) - 0.75), abs(_f(rho) - 0.25)) > E_rho
        d = mpf(float(delta))
        if rho > 0.75:
            grow = 3 * hn > d
            out["branch"] = "grow"; out["delta_next"] = Val(3 * hn, E_3h) if grow else Val(d, 0.0)
            out["max_decided"] = abs(_f(3 * hn - d)) > E_3h
        elif rho < 0.25:
            out["branch"] = "halve"; out["delta_next"] = Val(d / 2, 0.0); out["max_decided"] = True
        else:
            out["branch"] = "keep"; out["delta_next"] = Val(d, 0.0); out["max_decided"] = True
    return out


def dogleg(S, h_gn, delta, chi_old=None, chi_new=None):
    """one dogleg trial on the system S with the Gauss-Newton step h_gn (packed over S's scalars): dict of Val and per-scalar arrays"""
    n = S.nf; b = S.b; g = np.asarray(h_gn, dtype=np.float64); ab = np.abs(b); d = mpf(float(delta))
    Hb, SHb = S.mul(b); eHb = S.mul_bound(SHb)
    bb = xdot(b, b); bHb = S.quad(b, b); bg = xdot(b, g); gg = xdot(g, g); bHg = S.quad(b, g); gHg = S.quad(g, g)
    E_bb = n * U * _f(bb); E_bHb = float((ab * eHb).sum() + n * U * (ab * np.abs(Hb)).sum())
    ok = MP.isfinite(bHb) and bHb > 0
    alpha = bb / bHb if ok else mpf(0)
    E_alpha = _f(alpha) * (E_bb / _f(bb) + E_bHb / _f(bHb) + U) if ok else 0.0
    out = dict(Hb=(Hb, eHb), bb=Val(bb, E_bb), bHb=Val(bHb, E_bHb), alpha=Val(alpha, E_alpha), alpha_decided=abs(_f(bHb)) > E_bHb)
    hs = _f(alpha) * b; a = g - hs; ahs, aa = np.abs(hs), np.abs(a)
    e_s = ab * E_alpha + U * ahs; e_a = e_s + U * aa
    ss = alpha * alpha * bb; cc = alpha * bg - ss; qq = gg - 2 * alpha * bg + ss
    E_gg = n * U * _f(gg); E_ss = float(2 * (ahs * e_s).sum() + n * U * _f(ss))
    E_cc = float((aa * e_s + ahs * e_a).sum() + n * U * (ahs * aa).sum()); E_qq = float(2 * (aa * e_a).sum() + n * U * _f(qq))
    gn, sd = MP.sqrt(gg), MP.sqrt(ss)
    E_gn = E_gg / (2 * _f(gn)) + U * _f(gn) if gn > 0 else 0.0; E_sd = E_ss / (2 * _f(sd)) + U * _f(sd) if sd > 0 else 0.0
    out.update(gg=Val(gg, E_gg), ss=Val(ss, E_ss), cc=Val(cc, E_cc), qq=Val(qq, E_qq), gn=Val(gn, E_gn), sd=Val(sd, E_sd), h_sd=(hs, e_s))
    kind = GN if gn < d else (SD if sd > d else DL)
    out["kind"] = kind
    out["kind_decided"] = abs(_f(gn - d)) > E_gn and (kind == GN or abs(_f(sd - d)) > E_sd)
    if kind == GN:
        s, t = mpf(0), mpf(1); e_h = np.zeros(S.n)
    elif kind == SD:
        sc = d / sd; E_sc = _f(sc) * (E_sd / _f(sd) + U); s, t = sc * alpha, mpf(0)
        e_h = ahs * E_sc + _f(sc) * e_s
        out["scale"] = Val(sc, E_sc)
    else:
        m = d * d - ss; E_m = U * _f(d * d) + E_ss + U * abs(_f(m))
        r = cc * cc + qq * m; E_r = 2 * abs(_f(cc)) * E_cc + U * _f(cc * cc) + abs(_f(m)) * E_qq + _f(qq) * E_m + U * abs(_f(qq * m)) + U * abs(_f(r))
        disc = MP.sqrt(r); E_disc = E_r / (2 * _f(disc)) + U * _f(disc) if disc > 0 else 0.0
        if qq > 0:
            num, den = -cc + disc, cc + disc
            beta_neg = num / qq; beta_pos = m / den if den != 0 else beta_neg
            beta = beta_neg if cc <= 0 else beta_pos; ab_ = abs(_f(beta))
            Eb_neg = (E_cc + E_disc + U * abs(_f(num))) / _f(qq) + ab_ * E_qq / _f(qq) + U * ab_
            Eb_pos = (E_m / abs(_f(den)) + ab_ * (E_cc + E_disc + U * abs(_f(den))) / abs(_f(den)) + U * ab_) if den != 0 else math.inf
            cc_decided = abs(_f(cc)) > E_cc
            E_beta = (Eb_neg if cc <= 0 else Eb_pos) if cc_decided else max(Eb_neg, Eb_pos)
        else:
            beta = beta_neg = beta_pos = mpf(0); E_beta = 0.0; cc_decided = True
        out.update(m=Val(m, E_m), disc=Val(disc, E_disc), beta=Val(beta, E_beta), beta_neg=beta_neg, beta_pos=beta_pos, cc_decided=cc_decided)
        s, t = (1 - beta) * alpha, beta
        e_h = e_s + aa * E_beta + abs(_f(beta)) * e_a + U * abs(_f(beta)) * aa
    h = [mpf(0)] * S.n
    for i in np.flatnonzero(S.free):
        h[i] = s * mpf(float(b[i])) + t * mpf(float(g[i]))
    hf = np.array([float(v) for v in h])
    if kind != GN:
        e_h = e_h + U * np.abs(hf)
    out["h"] = h; out["h_f"] = hf; out["e_h"] = e_h; out["st"] = (s, t)
    hh = s * s * bb + 2 * s * t * bg + t * t * gg; hHh = s * s * bHb + 2 * s * t * bHg + t * t * gHg; bh = s * bb + t * bg
    out.update(gain_terms(S, hHh, bh, hh, hf, e_h, delta, chi_old, chi_new))
    return out


def gain_of_step(S, h, delta, chi_old, chi_new):
    """gain, rho, delta_next of a step that is given as fp64 numbers (the device's own h_dl): no bound on h itself"""
    h = np.asarray(h, dtype=np.float64)
    return gain_terms(S, S.quad(h, h), xdot(S.b, h), xdot(h, h), h, np.zeros(S.n), delta, chi_old, chi_new)


def norm_of_step(h, e_h):
    """|h| of fp64 numbers h, exactly, and what per-scalar bounds e_h on h allow it to be off by"""
    hh = xdot(h, h); hn = MP.sqrt(hh)
    return Val(hn, float((np.abs(h) * e_h).sum() / _f(hn)) if hn > 0 else 0.0)


def check_vector(got, ref, tag=""):
    """every free scalar of `got` within e_h of the reference's h; returns (worst err / bound, entries with a positive bound)"""
    worst = 0.0; n = 0
    for i, (v, hx, e) in enumerate(zip(got, ref["h"], ref["e_h"])):
        err = float(abs(mpf(float(v)) - hx))
        if e > 0:
            worst = max(worst, err / e); n += 1
        assert err <= e, "%s scalar %d: |err| %.3e > bound %.3e" % (tag, i, err, e)
    return worst, n


# ---------------------------------------------------------------- Levenberg-Marquardt
def lm_update(lam, rho):
    """lambda * max(1/3, min(1 - (2 rho - 1)^3, 2/3)) for rho = Val: (Val, which = "2/3" | "1/3" | "cubic", decided)"""
    lam_ = mpf(float(lam)); r = rho.value
    t = 2 * r - 1; E_t = 2 * rho.bound + U * abs(_f(t))
    t3 = t * t * t; E_t3 = 3 * _f(t * t) * E_t + 2 * U * abs(_f(t3))
    al = 1 - t3; E_al = E_t3 + U * abs(_f(al))
    lo, hi = mpf(1.0 / 3.0), mpf(2.0 / 3.0)
    decided = min(abs(_f(al - hi)), abs(_f(al - lo))) > E_al
    if al >= hi:
        return Val(mpf(float(lam) * (2.0 / 3.0)), 0.0), "2/3", decided
    if al <= lo:
        return Val(mpf(float(lam) * (1.0 / 3.0)), 0.0), "1/3", decided
    v = lam_ * al
    return Val(v, float(lam) * E_al + U * _f(v)), "cubic", decided


def lm(dx, b, lam, chi_old, chi_new, free=None):
    """scale, rho, verdict and the lambda update of one LM trial from the increment dx, b (flat, the same order), lambda, chi_old, chi_new"""
    dx = np.asarray(dx, dtype=np.float64).reshape(-1); b = np.asarray(b, dtype=np.float64).reshape(-1)
    if free is not None:
        dx = np.where(free, dx, 0.0); b = np.where(free, b, 0.0)
    n = int(free.sum()) if free is not None else len(dx); lam_ = mpf(float(lam))
    scale = lam_ * xdot(dx, dx) + xdot(dx, b) + mpf(1e-3)
    inner = float(lam) * dx + b; adx = np.abs(dx)
    E = float(U * (float(lam) * dx * dx + 2 * adx * np.abs(inner)).sum() + (n - 1) * U * (adx * np.abs(inner)).sum() + U * abs(_f(scale)))
    rho = (mpf(float(chi_old)) - mpf(float(chi_new))) / scale; E_rho = abs(_f(rho)) * (2 * U + E / abs(_f(scale)))
    out = dict(scale=Val(scale, E), rho=Val(rho, E_rho), accept=bool(rho > 0 and math.isfinite(chi_new)), accept_decided=abs(_f(rho)) > E_rho)
    if out["accept"]:
        out["lambda_next"], out["clip"], out["clip_decided"] = lm_update(lam, out["rho"])
    else:
        out["lambda_next"], out["clip"], out["clip_decided"] = Val(mpf(float(lam) * 2.0), 0.0), "rejected", True
    return out


DIAG3 = (0, 4, 8); DIAG2 = (0, 3)


def max_diag(B, g):
    """(max |H_jj| over the free scalars of an export, ("pose" | "landmark", vertex) where it sits)"""
    N, M = len(B["Hpp_diag"]), len(B["Hll_diag"]); fp, fl = hr.masks(g, N, M)
    dp = np.where(fp[:, None], np.abs(np.asarray(B["Hpp_diag"])[:, DIAG3]), 0.0); dl = np.where(fl[:, None], np.abs(np.asarray(B["Hll_diag"])[:, DIAG2]), 0.0)
    mp_, ml_ = dp.max(initial=0.0), dl.max(initial=0.0)
    if mp_ >= ml_:
        return float(mp_), ("pose", int(np.argmax(dp.max(axis=1))))
    return float(ml_), ("landmark", int(np.argmax(dl.max(axis=1))))


def slot_bound(g, M, H_jj, lam):
    """2 k u (H_jj + lambda) per landmark diagonal scalar [M, 2], k = the landmark's observation edges (>= its slots)"""
    k = np.maximum(np.bincount(np.asarray(g["pl_l"], dtype=np.int64), minlength=M), 1)
    return 2.0 * k[:, None] * U * (np.abs(H_jj) + lam)
