"""The exact terms of the two side passes (TEST-ONLY; mpmath, 60 digits) and the entry-wise bound they are held to: the prior edges
(k_prior_pass) and the polar observation edges (k_polar_pose, k_polar_lm, k_polar_edge_chi2).

Written from the formulas of include/graphslam.h (prior and polar sections) — not from the kernels, not from the numpy checkers:
    pose prior       e = (R_z^T (t - t_z), normalize(theta - z_theta)),  J = diag(R_z^T, 1)
    XY prior         the pose prior with z_theta = 0 and Omega in the upper-left 2 x 2
    landmark prior   e = l - z,  J = I
    range-bearing    d = x_p^-1 . l,  r = |d|,  beta = atan2(dy, dx),  e = (r - z_r, normalize(beta - z_beta)),
                     J_d = [[dx/r, dy/r], [-dy/r^2, dx/r^2]],  B = J_d R^T,  A = [-B | (0, -1)^T]
    bearing-only     the range-bearing edge with z_r = 0 and Omega = [[0, 0], [0, omega]]
    every term       H += J^T W J,  b -= J^T W e,  chi2 += rho(s),  s = e^T W e.  The observation kind's robust kernel applies to polar edges,
                     never to priors.  A fixed endpoint stays out of H, an edge between two fixed vertices out of chi2, a prior on a fixed
                     vertex out of everything; r == 0 and an inactive edge contribute nothing.
All inputs are the fp64 numbers the handle is given, taken exactly; cos, sin, atan2, sqrt are mpmath's.

accumulate() adds the terms to a lin_exact_ref.Exact on top of lin_exact_ref.linearize of the graph with its carriers (z = 0, information 0):
one object then describes gs_export_system, gs_chi2, the per-edge s and weight of gs_get_edge_chi2 and gs_get_prior_chi2.

Magnitudes S, in the spirit of lin_exact_ref (every elementary product by absolute value):
    prior     the host stores the INVERSE measurement, -R_z^T t_z rounded in fp64, with libm's cos / sin of z_theta, so e_t is a sum of four
              rounded products: S = |c_z| (|x| + |z_x|) + |s_z| (|y| + |z_y|).  S of e_theta = |theta| + |z_theta| + 2 pi per wrap (the device
              subtracts the fp64 2 pi: once where the estimate's own heading lies outside [-pi, pi), once where the difference does).
    polar     nonlinear in d, so S carries the error of d to first order (what lin_exact_ref.robust does for a weight: S_s1).  With d~ the
              magnitude of d (mag_pl with z = 0; the error of d is at most 7 u d~):
                  S_r    = r + (|dx| d~x + |dy| d~y) / r                   S_beta = |beta| + (|dy| d~x + |dx| d~y) / r^2
                  S(dx/r)   = |dx| / r + d~x / r + |dx| (|dx| d~x + |dy| d~y) / r^3          (dy / r likewise)
                  S(dy/r^2) = |dy| / r^2 + d~y / r^2 + 2 |dy| (|dx| d~x + |dy| d~y) / r^4    (dx / r^2 likewise)
              and these go through B, A, the products and s as any magnitude does.  The second-order rest of a function f of d is at most
              |f''| |dd|^2 / 2 with |f''| <= 3 / r^k (k = 1 for r, 2 for beta and dx / r, 3 for dy / r^2) and |dd| <= 7 u (d~x + d~y): each S gets
              4 * 7 u (d~x + d~y)^2 / r^k on top, and the reference refuses an edge with 7 u (d~x + d~y) / r > 1e-3, where "second order" ends.
              A wrapped bearing adds 2 pi; a landmark on the negative x-axis of the pose frame (beta = +-pi by the sign of a zero) counts as wrapped.

The bound stays |got - exact| <= C(n) u S, C(n) = 2 (L + n), u = 2^-53, with L per entry the longest chain among the terms summed into it
(Exact.L).  The count of roundings, one line per step; device cos / sin 4 ulp, atan2 6 ulp, log 3 ulp (the OpenCL fp64 bounds), sqrt and
division correctly rounded (csrc/Makefile builds with -O3 and no fast-math flag), the host's libm cos / sin 1 ulp:
    pose prior
      e_t      libm cos / sin 1, product 1, the inner addition (host for z, device for x) 1, the outer addition 1     =  4
      e_theta  normalising the estimate's heading: the fp64 2 pi 1, product 1, subtraction 1 = 3; the addition 1; normalising the sum 3 =  7
      W e      e 7, product 1, two additions 2                                                                       = 10
      J^T W e  J 1, W e 10, product 1, addition 1                                                                    = 13
      J^T W J  W J: J 1, product 1, addition 1 = 3;  J 1, W J 3, product 1, addition 1                                =  6
      s        e 7, W e 10, product 1, two additions 2                                                               = 20     <- L_PRIOR
    landmark prior   e 1, W e 3, s 6; H = Omega exactly                                                                      (<= L_PRIOR)
    polar edge
      d        cos / sin 4, product 1, inner addition 1, outer addition 1                                            =  7
      r        d 7, square 1, addition 1, sqrt 1                                                                     = 10
      beta     d 7, atan2 6                                                                                          = 13
      e        e_r: r 10, subtraction 1 = 11;  e_beta: beta 13, subtraction 1, a wrap 3                              = 17
      J_d      r 10 (r^2: 9), division 1                                                                             = 11
      B        J_d 11, cos / sin 4, product 1, addition 1                                                            = 17     (A = [-B | (0, -1)^T]: 17)
      W B      B 17, product 1, addition 1                                                                           = 19     (W e: e 17, 2 = 19)
      B^T W B  B 17, W B 19, product 1, addition 1                                                                   = 38     (A^T W A, A^T W B, b: the same)
      s        e 17, W e 19, product 1, addition 1                                                                   = 38     <- L_POLAR
    robust     weight: s 38 (through |w'| S_s1), delta^2 1, division / addition / division or sqrt / division 3       = 42     <- L_WEIGHT
               a term: the plain term 38, the weight 42, the product Omega * w 1                                    = 81     <- L_POLAR_ROBUST
               rho: s 38, delta^2 1, division 1, addition 1, log 3, product 1 = 45 (Cauchy); sqrt 1, two products 2, subtraction 1 (Huber): below 81
    sums       as in lin_exact_ref: n terms, n - 1 additions in whatever grouping (the passes ADD their sums to what the linearisation left;
               the carrier of a polar edge counts as a term), the chi2 partials' second level 1;  together L + n, doubled.
The constants come from this count alone; what the device is measured at is in test_gpu_side_exact.py's docstring.

Refusals (assertions, as lin_exact_ref.robust at a kernel's branch point): an angle error within 1e-6 of +-pi; a Huber s within 1e-6
relative of delta^2; r below 1e-6 unless r is exactly 0."""
import numpy as np

import lin_exact_ref as lx
import robust_ref as rr

MP, mpf, U, ZERO = lx.MP, lx.mpf, lx.U, lx.ZERO
mm, tr, mabs, scal, col, fl = lx.mm, lx.tr, lx.mabs, lx.scal, lx.col, lx.fl
L_PRIOR, L_POLAR, L_WEIGHT, L_POLAR_ROBUST = 20, 38, 42, 81
L_WEIGHT_CART = 38                                     # lin_exact_ref's count of a Cartesian edge's weight
D_ROUNDINGS = 7
ONE = mpf(1)


def _clear_of_pi(a, what):
    k = a / MP.pi
    assert abs(abs(k - 2 * MP.floor(k / 2) - 1)) > 1e-6 / MP.pi, ("an angle error sits on the wrap's branch point", what, float(a))


def _quad(e, em, Js, Jms, W, kernel, L):
    """per edge: s, S_s, (w, S_w), (rho, S_rho), the blocks J_a^T W J_b and -J_a^T W e with their magnitudes (lin_exact_ref's quad, with the
    chain length L of this edge type in the second-order rest of S_s1)"""
    Wm = mabs(W)
    s = mm(tr(col(e)), mm(W, col(e)))[0][0]; S_s = mm(tr(col(em)), mm(Wm, col(em)))[0][0]
    ea = col([abs(v) for v in e])
    S_s1 = 2 * mm(tr(col(em)), mm(Wm, ea))[0][0] + mm(tr(ea), mm(Wm, ea))[0][0] + L * U * S_s
    w, rho, S_w, S_rho = lx.robust(kernel, s, S_s, S_s1)
    H = {}; b = []
    for a in range(len(Js)):
        b.append((fl(scal(mm(tr(Js[a]), mm(W, col(e))), -w)), fl(scal(mm(tr(Jms[a]), mm(Wm, col(em))), S_w))))
        for c in range(a, len(Js)):
            H[a, c] = (fl(scal(mm(tr(Js[a]), mm(W, Js[c])), w)), fl(scal(mm(tr(Jms[a]), mm(Wm, Jms[c])), S_w)))
    return dict(s=s, S_s=S_s, w=w, S_w=S_w, rho=rho, S_rho=S_rho, H=H, b=b)


# ---- the polar edge
def polar_geometry(xp, l):
    """d = x_p^-1 . l, r, beta, J_d and the magnitudes (S_d, S_r, S_beta, S_Jd); None where r == 0 exactly"""
    c, s = MP.cos(xp[2]), MP.sin(xp[2])
    ux, uy = l[0] - xp[0], l[1] - xp[1]
    dx, dy = c * ux + s * uy, -s * ux + c * uy
    if dx == 0 and dy == 0:
        return None
    dm = lx.mag_pl(xp, l, [ZERO, ZERO])[0]
    r2 = dx * dx + dy * dy; r = MP.sqrt(r2)
    assert r >= 1e-6, ("a range below 1e-6 that is not exactly zero", float(r))
    assert D_ROUNDINGS * U * (dm[0] + dm[1]) / r < 1e-3, ("the error of d is not small against r", float(r))
    q = 4 * D_ROUNDINGS * U * (dm[0] + dm[1]) ** 2                                    # second-order rest, to be divided by r^k
    p1 = abs(dx) * dm[0] + abs(dy) * dm[1]                                            # |d|^T d~
    beta = MP.atan2(dy, dx)
    S_r = r + p1 / r + q / r
    S_beta = abs(beta) + (abs(dy) * dm[0] + abs(dx) * dm[1]) / r2 + q / r2
    Jd = [[dx / r, dy / r], [-dy / r2, dx / r2]]
    S_Jd = [[abs(dx) / r + dm[0] / r + abs(dx) * p1 / (r * r2) + q / r2, abs(dy) / r + dm[1] / r + abs(dy) * p1 / (r * r2) + q / r2],
            [abs(dy) / r2 + dm[1] / r2 + 2 * abs(dy) * p1 / (r2 * r2) + q / (r * r2), abs(dx) / r2 + dm[0] / r2 + 2 * abs(dx) * p1 / (r2 * r2) + q / (r * r2)]]
    return dict(d=(dx, dy), dm=dm, r=r, beta=beta, S_r=S_r, S_beta=S_beta, Jd=Jd, S_Jd=S_Jd, c=c, s=s, on_negative_axis=(dy == 0 and dx < 0))


def polar_edge(xp, l, z, W, kernel, cartesian_route=False):
    """everything one polar edge gives (_quad's dict, the vertices in the order pose, landmark) with `unwrapped`, the angle beta - z_beta
    before it is normalised, and `geo`; None where r == 0"""
    geo = polar_geometry(xp, l)
    if geo is None:
        return None
    a = geo["beta"] - z[1]
    _clear_of_pi(a, "beta - z_beta")
    wrapped = a >= MP.pi or a < -MP.pi or geo["on_negative_axis"]
    e = [geo["r"] - z[0], lx.normalize(a)]
    em = [geo["S_r"] + abs(z[0]), geo["S_beta"] + abs(z[1]) + (2 * MP.pi if wrapped else ZERO)]
    c, s = geo["c"], geo["s"]
    Rt = [[c, s], [-s, c]]
    B = mm(geo["Jd"], Rt); Bm = mm(geo["S_Jd"], mabs(Rt))
    A = [[-B[0][0], -B[0][1], ZERO], [-B[1][0], -B[1][1], -ONE]]; Am = [[Bm[0][0], Bm[0][1], ZERO], [Bm[1][0], Bm[1][1], ONE]]
    if cartesian_route:             # A's last column as J_d (dy, -dx)^T: (dx dy - dy dx) / r = 0 by a cancellation the formula itself does not have
        dx, dy = geo["d"]
        Am[0][2] = 2 * abs(dx) * abs(dy) / geo["r"]
    out = _quad(e, em, (A, B), (Am, Bm), W, kernel, L_POLAR)
    out.update(unwrapped=a, wrapped=wrapped, geo=geo, e=e, em=em, A=A, B=B)
    return out


# ---- the priors
def pose_prior(x, z, W):
    cz, sz = MP.cos(z[2]), MP.sin(z[2])
    ux, uy = x[0] - z[0], x[1] - z[1]
    a = x[2] - z[2]
    _clear_of_pi(a, "theta - z_theta")
    xn = lx.normalize(x[2]); a2 = xn - z[2]
    wraps = int(xn != x[2]) + int(a2 >= MP.pi or a2 < -MP.pi)
    e = [cz * ux + sz * uy, -sz * ux + cz * uy, lx.normalize(a)]
    ax, ay = abs(x[0]) + abs(z[0]), abs(x[1]) + abs(z[1])
    em = [abs(cz) * ax + abs(sz) * ay, abs(sz) * ax + abs(cz) * ay, abs(x[2]) + abs(z[2]) + 2 * MP.pi * wraps]
    J = [[cz, sz, ZERO], [-sz, cz, ZERO], [ZERO, ZERO, ONE]]
    out = _quad(e, em, (J,), (mabs(J),), W, rr.NONE, L_PRIOR)
    out.update(unwrapped=a, wraps=wraps, e=e)
    return out


def lm_prior(l, z, W):
    e = [l[0] - z[0], l[1] - z[1]]; em = [abs(l[0]) + abs(z[0]), abs(l[1]) + abs(z[1])]
    J = [[ONE, ZERO], [ZERO, ONE]]
    out = _quad(e, em, (J,), (J,), W, rr.NONE, L_PRIOR)
    out.update(e=e)
    return out


def _v(a):
    return [mpf(float(t)) for t in np.asarray(a, dtype=np.float64).reshape(-1)]


def accumulate(X, g, polar=None, pri=None, kernels=None, off=(), poses=None, lms=None, perturb=None, cartesian_route=False):
    """adds the polar set's and the prior set's terms (polar_ref / prior_ref layouts) to X = lin_exact_ref.linearize(carriers); off: inactive
    observation edges (polar ones).  Fills X.s_pl / X.S_s_pl at the polar edges, X.w_pl / X.S_w_pl / X.L_w_pl for every observation edge,
    X.prior_s / X.prior_S per kind, and X.polar (per polar edge: its dict or None) for the census."""
    k_pl = (kernels or {}).get("observation", rr.NONE)
    robust_on = k_pl[0] != "none"
    P = lx._m(g["pose_est"] if poses is None else poses, (-1, 3)); Lm = lx._m(g["lm_est"] if lms is None else lms, (-1, 2))
    pf = np.zeros(len(P), dtype=bool); pf[np.asarray(g["fixed_poses"], dtype=np.int64)] = True
    lf = np.zeros(len(Lm), dtype=bool); lf[np.asarray(g["fixed_landmarks"], dtype=np.int64)] = True
    off = set(int(k) for k in off)
    assert polar is not None or not off
    assert all(k in set(int(i) for i in polar["idx"]) for k in off), "inactive Cartesian edges are not modelled here"
    E = len(g["pl_p"])
    # the weight of every observation edge: Cartesian ones from lin_exact_ref's own functions
    X.w_pl = [ONE] * E; X.S_w_pl = np.ones(E); X.L_w_pl = np.full(E, float(L_WEIGHT_CART))
    is_polar = np.zeros(E, dtype=bool)
    if polar is not None:
        is_polar[polar["idx"]] = True
    if robust_on:
        Z = lx._m(g["pl_z"], (-1, 2)); Wc = np.asarray(g["pl_info"], dtype=np.float64).reshape(-1, 2, 2)
        for k in np.flatnonzero(~is_polar):
            p, l = int(g["pl_p"][k]), int(g["pl_l"][k])
            e = lx.err_pl(P[p], Lm[l], Z[k]); em, Am, Bm = lx.mag_pl(P[p], Lm[l], Z[k]); A, B = lx.jac_pl(P[p], Lm[l])
            t = _quad(e, em, (A, B), (Am, Bm), lx._m(Wc[k], (2, 2)), k_pl, lx.L_PLAIN)
            X.w_pl[k] = t["w"]; X.S_w_pl[k] = float(t["S_w"])
    X.L_s_pl = np.full(E, float(lx.L_PLAIN)); X.polar = []
    L_term = L_POLAR_ROBUST if robust_on else L_POLAR
    for n, k in enumerate(polar["idx"] if polar is not None else ()):
        k = int(k); p, l = int(g["pl_p"][k]), int(g["pl_l"][k])
        t = polar_edge(P[p], Lm[l], _v(polar["z"][n]), lx._m(polar["W"][n], (2, 2)), k_pl, cartesian_route)
        X.polar.append(t); X.L_s_pl[k] = L_POLAR; X.L_w_pl[k] = L_WEIGHT
        if t is None:
            X.s_pl[k] = ZERO; X.S_s_pl[k] = 0.0
            continue
        X.s_pl[k] = t["s"]; X.S_s_pl[k] = float(t["S_s"]); X.w_pl[k] = t["w"]; X.S_w_pl[k] = float(t["S_w"])
        if k in off:
            X.w_pl[k] = ZERO; X.S_w_pl[k] = 0.0
            continue
        if pf[p] and lf[l]:
            continue
        f = (ONE + mpf(perturb[1])) if perturb and perturb[0] == ("polar", n) else ONE
        X.chi2 += t["rho"] * f; X.chi2_Sm += t["S_rho"]; X.chi2_n += 1; X.chi2_terms.append(t["rho"]); X.chi2_tags.append("polar")
        X.chi2_L = max(X.chi2_L, L_term)
        H, b = t["H"], t["b"]
        if not pf[p]:
            X.add("Hpp_diag", p, [v * f for v in H[0, 0][0]], H[0, 0][1], L_term, "polar"); X.add("b_pose", p, [v * f for v in b[0][0]], b[0][1], L_term, "polar")
        if not lf[l]:
            X.add("Hll_diag", l, [v * f for v in H[1, 1][0]], H[1, 1][1], L_term, "polar"); X.add("b_lm", l, [v * f for v in b[1][0]], b[1][1], L_term, "polar")
        if not pf[p] and not lf[l]:
            X.add("Hpl", k, [v * f for v in H[0, 1][0]], H[0, 1][1], L_term, "polar")
    X.prior_s = dict(pose=[], landmark=[]); X.prior_S = dict(pose=[], landmark=[]); X.priors = dict(pose=[], landmark=[])
    for n, (p, z, W, _) in enumerate(pri["pose"] if pri is not None else ()):
        p = int(p); t = pose_prior(P[p], _v(z), lx._m(W, (3, 3)))
        X.prior_s["pose"].append(t["s"]); X.prior_S["pose"].append(float(t["S_s"])); X.priors["pose"].append(t)
        if pf[p]:
            continue
        f = (ONE + mpf(perturb[1])) if perturb and perturb[0] == ("pose prior", n) else ONE
        X.chi2 += t["s"] * f; X.chi2_Sm += t["S_s"]; X.chi2_n += 1; X.chi2_terms.append(t["s"]); X.chi2_tags.append("prior")
        X.add("Hpp_diag", p, [v * f for v in t["H"][0, 0][0]], t["H"][0, 0][1], L_PRIOR, "prior"); X.add("b_pose", p, [v * f for v in t["b"][0][0]], t["b"][0][1], L_PRIOR, "prior")
    for n, (l, z, W) in enumerate(pri["lm"] if pri is not None else ()):
        l = int(l); t = lm_prior(Lm[l], _v(z), lx._m(W, (2, 2)))
        X.prior_s["landmark"].append(t["s"]); X.prior_S["landmark"].append(float(t["S_s"])); X.priors["landmark"].append(t)
        if lf[l]:
            continue
        f = (ONE + mpf(perturb[1])) if perturb and perturb[0] == ("landmark prior", n) else ONE
        X.chi2 += t["s"] * f; X.chi2_Sm += t["S_s"]; X.chi2_n += 1; X.chi2_terms.append(t["s"]); X.chi2_tags.append("prior")
        X.add("Hll_diag", l, [v * f for v in t["H"][0, 0][0]], t["H"][0, 0][1], L_PRIOR, "prior"); X.add("b_lm", l, [v * f for v in t["b"][0][0]], t["b"][0][1], L_PRIOR, "prior")
    return X.finish()


def exact(g, polar=None, pri=None, kernels=None, off=(), poses=None, lms=None, perturb=None, cartesian_route=False):
    """the whole of gs_export_system, gs_chi2, gs_get_edge_chi2 and gs_get_prior_chi2 of a graph dict with a polar set and a prior set.
    perturb = ((pass, index), rel): that one edge's or prior's terms times (1 + rel) — a reference that is wrong on purpose.
    cartesian_route: the same values with the magnitudes of an evaluation through polar_ref.cartesianised, whose pose Jacobian holds
    J_d (dy, -dx)^T in its last column — (0, -1)^T after a cancellation of dx dy / r against itself, which the polar formula (and the
    device, which writes the 0 and the -1) does not have; every other magnitude is unchanged"""
    import polar_ref as plr
    gc = plr.carriers(g, polar) if polar is not None else g
    k = {"observation": kernels["observation"]} if kernels and "observation" in kernels else None
    X = lx.linearize(gc, k, poses, lms)
    return accumulate(X, g, polar, pri, kernels, off, poses, lms, perturb, cartesian_route)


def check_side(X, w_pl=None, prior_pose=None, prior_lm=None, tag=""):
    """the per-edge weight of gs_get_edge_chi2 and the per-prior values of gs_get_prior_chi2 against the bound; returns the worst ratios"""
    worst = {}
    for name, got, ex, S, c in (("w_pl", w_pl, X.w_pl, X.S_w_pl, 2.0 * (X.L_w_pl + 1.0)),
                                ("prior_pose", prior_pose, X.prior_s["pose"], np.asarray(X.prior_S["pose"]), 2.0 * (L_PRIOR + 1.0)),
                                ("prior_lm", prior_lm, X.prior_s["landmark"], np.asarray(X.prior_S["landmark"]), 2.0 * (L_PRIOR + 1.0))):
        if got is None:
            continue
        r = lx._ratio(lx._err(got, ex), np.asarray(S, dtype=np.float64)); c = np.broadcast_to(c, r.shape)
        if name == "w_pl":                                                       # a weight of exactly 1 (no kernel acts) or 0 (inactive) is exact
            fixed = np.array([v == 1 or v == 0 for v in ex]); r = np.where(fixed & (np.asarray(got) != np.array([float(v) for v in ex])), np.inf, r)
        worst[name] = float(r.max()) if len(r) else 0.0
        bad = np.flatnonzero(r > c)
        assert not len(bad), (tag, name, int(bad[0]), "err / (u S)", float(r[bad[0]]), "C", float(c[bad[0]]))
    return worst
