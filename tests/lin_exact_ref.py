"""Plain high-precision linearisation (TEST-ONLY; mpmath, 60 digits) and the entry-wise bound the linearisation pass is held to.

Written from g2o's formulas as DESIGN §2 states them — not from the kernels, not from the oracle:
    EdgeSE2          e = vec(z^-1 o (x_i^-1 o x_j)),  SE2^-1 = (R^T (-t), -theta),  a o b = (R_a t_b + t_a, theta_a + theta_b), angle normalised
                     J_i = Z [[-ci, -si, -si dx + ci dy], [si, -ci, -ci dx - si dy], [0, 0, -1]],  J_j = Z [[ci, si, 0], [-si, ci, 0], [0, 0, 1]],
                     Z = rot(z^-1) (3 x 3, 1 in the corner),  dx, dy = t_j - t_i                         (updates are additive: t += dt, theta += dtheta)
    EdgeSE2PointXY   e = (x_p^-1 . l) - z,  J_p = [[-c, -s, c ly - c py - s lx + s px], [s, -c, -s ly + s py - c lx + c px]],  J_l = R_p^T
    every edge       H += J^T W J,  b -= J^T W e,  chi2 += e^T W e;   a fixed vertex has zero rows and columns (its free neighbour keeps its own
                     diagonal share), an edge between two fixed vertices adds nothing, to chi2 either
    robust kernels   tests/robust_ref.py's definitions, evaluated here: W <- rho'(s) W, chi2 += rho(s), s = e^T W e
cos and sin are mpmath's, of the fp64 theta.  All inputs are the fp64 numbers the handle is given, taken exactly.

Every output entry comes with
    S   its magnitude: the same formula with every elementary product replaced by its absolute value — inside e too
        (|c lx| + |s ly| + |c px| + |s py| + |z|), so cancellation at kilometre coordinates enlarges S as it enlarges the rounding error;
    n   the number of edge terms summed into it.
A robust term w(s) t has S = S_t (w + |w'(s)| S_s1): the error of w is |w'| times that of s, plus its own roundings; S_s1 = 2 e~^T |W| |e| +
|e|^T |W| |e| (+ the second-order rest) bounds the error of s to first order — S_s = e~^T |W| e~ itself would leave every weight undetermined to 1e-7.

The bound:  |got - exact| <= C(n) u S,  u = 2^-53,  C(n) = 2 (L + n),  L = 34 (no robust kernel) or 71 (robust), from this count of the
roundings on the longest chain from an input to one edge's term (each counted as one u of the magnitude S; the device's cos and sin as
4 ulp each, the OpenCL bound):
    observation edge, quad_pl / edge_pl
      e        cos/sin 4, product 1, three additions 3                                              =  8
      A[.][2]  cos/sin 4, product 1, three additions 3                                              =  8
      W A      A 8, product 1, addition 1                                                           = 10
      A^T W A  A 8 (the factor: cos/sin enter a second time), W A 10, product 1, addition 1         = 20     (b_p: A 8, W e 10, 2 = 20)
      s        e 8, W e 10, product 1, addition 1                                                   = 20
    odometry edge, pp_incidence
      q = R_i^T (t_j - t_i)   cos/sin 4, difference 1, product 1, addition 1                        =  7
      a02 (lever arm)         q 7, cos/sin of z 4, product 1, addition 1                            = 13
      W a                     a 13, two products and the additions: 3                               = 16
      a^T W a (H theta-theta) a 13, W a 16, 3                                                       = 32
      e                       q 7 (in g2o's order: product 1, two additions 2, cos/sin 4), cos/sin of z 4, product 1, two additions 2 = 14
      W e                     e 14, 3                                                               = 17
      s                       e 14, W e 17, 3                                                       = 34     <- L without a robust kernel
    robust     weight: s 34 (through |w'| S_s1), delta^2 1, division / addition / division or sqrt / division 3 = 38;
               a term: the plain term 32, the weight 38, the product W * w 1                        = 71     <- L with one
    sums       n - 1 additions for n terms in whatever grouping (lanes of a pose, wave tile partials, wave and block sums of chi2), and 1 for
               the second level of the finalize pass;  together  L + n,  doubled as the solver tests' 64 (f_max + 2) u carries its own margin.

The bound can fail: `check_can_fail` multiplies one contributing edge's term of an entry by (1 + 1e-9); the unperturbed result must then violate
the bound at that entry wherever 1e-9 |term| > 2 C(n) u S, i.e. wherever ANY fp64 evaluation could tell (see check_can_fail).

The passes that run behind the linearisation and write into the same arrays (prior edges, polar observation edges) add their terms to the
same Exact through add(..., L, tag) with the L of their own rounding count (tests/side_exact_ref.py): an entry's constant is then
2 (L + n) with L the longest chain among its terms — for an entry that holds only the linearisation's terms, what it was."""
import numpy as np
import mpmath

import robust_ref as rr

MP = mpmath.mp.clone()
MP.dps = 60
mpf = MP.mpf
U = 2.0 ** -53
L_PLAIN, L_ROBUST = 34, 71
ARRAYS = ("Hpp_diag", "Hll_diag", "Hpp_off", "Hpl", "b_pose", "b_lm")
WIDTH = dict(Hpp_diag=9, Hll_diag=4, Hpp_off=9, Hpl=6, b_pose=3, b_lm=2)
REL = 1e-9
ZERO = mpf(0)


def C(n, robust=False):
    """the derived constant of the bound for an entry summed from n edge terms (module docstring)"""
    return 2.0 * ((L_ROBUST if robust else L_PLAIN) + np.asarray(n, dtype=np.float64))


# ---- small dense helpers on lists of lists of mpf
def mm(A, B):
    return [[sum((A[r][t] * B[t][c] for t in range(len(B))), ZERO) for c in range(len(B[0]))] for r in range(len(A))]


def tr(A):
    return [list(r) for r in zip(*A)]


def mabs(A):
    return [[abs(v) for v in r] for r in A]


def scal(A, w):
    return [[v * w for v in r] for r in A]


def col(v):
    return [[x] for x in v]


def fl(A):
    return [v for r in A for v in r]


def _m(a, shape):
    a = np.asarray(a, dtype=np.float64).reshape(shape)
    return [[mpf(float(v)) for v in r] for r in a]


def normalize(th):
    """angle into [-pi, pi) (g2o normalize_theta)"""
    twopi = 2 * MP.pi
    while th >= MP.pi:
        th -= twopi
    while th < -MP.pi:
        th += twopi
    return th


# ---- the two error functions and their Jacobians (arguments: lists of mpf)
def err_pl(xp, l, z):
    c, s = MP.cos(xp[2]), MP.sin(xp[2])
    dx, dy = l[0] - xp[0], l[1] - xp[1]
    return [c * dx + s * dy - z[0], -s * dx + c * dy - z[1]]


def jac_pl(xp, l):
    c, s = MP.cos(xp[2]), MP.sin(xp[2])
    dx, dy = l[0] - xp[0], l[1] - xp[1]
    return [[-c, -s, c * dy - s * dx], [s, -c, -s * dy - c * dx]], [[c, s], [-s, c]]


def mag_pl(xp, l, z):
    """(e~, A~, B~): the magnitudes, every elementary product by absolute value"""
    c, s = abs(MP.cos(xp[2])), abs(MP.sin(xp[2]))
    px, py, lx, ly = abs(xp[0]), abs(xp[1]), abs(l[0]), abs(l[1])
    e = [c * lx + s * ly + c * px + s * py + abs(z[0]), s * lx + c * ly + s * px + c * py + abs(z[1])]
    A = [[c, s, c * ly + c * py + s * lx + s * px], [s, c, s * ly + s * py + c * lx + c * px]]
    return e, A, [[c, s], [s, c]]


def err_pp(xi, xj, z):
    ci, si = MP.cos(xi[2]), MP.sin(xi[2]); cz, sz = MP.cos(z[2]), MP.sin(z[2])
    dx, dy = xj[0] - xi[0], xj[1] - xi[1]
    qx, qy = ci * dx + si * dy - z[0], -si * dx + ci * dy - z[1]              # (x_i^-1 o x_j).t - z.t
    return [cz * qx + sz * qy, -sz * qx + cz * qy, normalize(xj[2] - xi[2] - z[2])]


def jac_pp(xi, xj, z):
    ci, si = MP.cos(xi[2]), MP.sin(xi[2]); cz, sz = MP.cos(z[2]), MP.sin(z[2])
    dx, dy = xj[0] - xi[0], xj[1] - xi[1]
    Z = [[cz, sz, ZERO], [-sz, cz, ZERO], [ZERO, ZERO, mpf(1)]]
    Ji = [[-ci, -si, -si * dx + ci * dy], [si, -ci, -ci * dx - si * dy], [ZERO, ZERO, mpf(-1)]]
    Jj = [[ci, si, ZERO], [-si, ci, ZERO], [ZERO, ZERO, mpf(1)]]
    return mm(Z, Ji), mm(Z, Jj)


def mag_pp(xi, xj, z):
    ci, si = abs(MP.cos(xi[2])), abs(MP.sin(xi[2])); cz, sz = abs(MP.cos(z[2])), abs(MP.sin(z[2]))
    ax, ay = abs(xj[0]) + abs(xi[0]), abs(xj[1]) + abs(xi[1])
    qx, qy = ci * ax + si * ay + abs(z[0]), si * ax + ci * ay + abs(z[1])
    e = [cz * qx + sz * qy, sz * qx + cz * qy, abs(xj[2]) + abs(xi[2]) + abs(z[2])]
    Z = [[cz, sz, ZERO], [sz, cz, ZERO], [ZERO, ZERO, mpf(1)]]
    Ji = [[ci, si, si * ax + ci * ay], [si, ci, ci * ax + si * ay], [ZERO, ZERO, mpf(1)]]
    Jj = [[ci, si, ZERO], [si, ci, ZERO], [ZERO, ZERO, mpf(1)]]
    return e, mm(Z, Ji), mm(Z, Jj)


def robust(kernel, s, S_s, S_s1):
    """(w, rho, S_w, S_rho) of tests/robust_ref.py's kernels at s; asserts s stays 1e-6 relative clear of delta^2 (no branch can flip).
    S_s: the magnitude of s (of rho = s without a kernel); S_s1: the first-order magnitude of the error of s, which is what a weight sees"""
    name, delta = kernel
    if name == "none":
        return mpf(1), s, mpf(1), S_s
    d = mpf(float(delta)); d2 = d * d
    assert abs(s - d2) > 1e-6 * d2, ("an edge sits on the kernel's branch point", float(s), float(d2))
    if name == "huber":
        if s <= d2:
            return mpf(1), s, mpf(1), S_s
        r = MP.sqrt(s); w = d / r
        return w, 2 * r * d - d2, w + w / (2 * s) * S_s1, w * S_s1 + abs(2 * r * d) + d2
    if name == "cauchy":
        w = 1 / (1 + s / d2); rho = d2 * MP.log(1 + s / d2)
        return w, rho, w + w * w / d2 * S_s1, w * S_s1 + rho
    raise ValueError(name)


class Exact:
    """val[name]: flat list of mpf in export_system's layout, S[name] / n[name]: float / int arrays of the same length, terms[name][flat index]:
    the edge terms summed into the entry; chi2 (val, S, n, terms); s_pp / s_pl with S_s_pp / S_s_pl per edge (every edge, as gs_get_edge_chi2)."""

    def __init__(self, sizes, robust_on):
        self.robust = robust_on
        self.val = {k: [ZERO] * (sizes[k] * WIDTH[k]) for k in ARRAYS}
        self.Sm = {k: [ZERO] * (sizes[k] * WIDTH[k]) for k in ARRAYS}
        self.n = {k: np.zeros(sizes[k] * WIDTH[k], dtype=np.int64) for k in ARRAYS}
        self.terms = {k: {} for k in ARRAYS}
        self.chi2, self.chi2_Sm, self.chi2_n, self.chi2_terms = ZERO, ZERO, 0, []
        self.s_pp, self.s_pl, self.S_s_pp, self.S_s_pl = [], [], [], []
        # L of the bound per entry: the longest chain among the terms summed into it.  The linearisation's own terms have L_PLAIN / L_ROBUST
        # (the module docstring); a side pass (tests/side_exact_ref.py) passes the L of its own count and a tag naming the pass
        self.base_L = L_ROBUST if robust_on else L_PLAIN
        self.L = {k: np.zeros(sizes[k] * WIDTH[k], dtype=np.int64) for k in ARRAYS}
        self.tags = {k: {} for k in ARRAYS}
        self.chi2_L, self.chi2_tags = self.base_L, []
        self.L_s_pl = None                                         # per observation edge, where a side pass has a longer chain to s than L_PLAIN

    def add(self, name, row, vals, mags, L=None, tag=None):
        w = WIDTH[name]
        for t, (v, m) in enumerate(zip(vals, mags)):
            k = row * w + t
            self.val[name][k] += v; self.Sm[name][k] += m; self.n[name][k] += 1
            self.L[name][k] = max(self.L[name][k], self.base_L if L is None else L)
            self.terms[name].setdefault(k, []).append(v); self.tags[name].setdefault(k, []).append(tag)

    def bound(self, name):
        """C(n) = 2 (L + n) per entry of an array"""
        return 2.0 * (self.L[name] + self.n[name]).astype(np.float64)

    def chi2_bound(self):
        return 2.0 * (self.chi2_L + self.chi2_n)

    def finish(self):
        self.S = {k: np.array([float(v) for v in self.Sm[k]]) for k in ARRAYS}
        self.chi2_S = float(self.chi2_Sm)
        return self


def linearize(g, kernels=None, poses=None, lms=None):
    """the exact linearisation of a graph dict (conftest layout) at its estimates, or at the given ones"""
    kernels = kernels or {}
    k_pp, k_pl = kernels.get("odometry", rr.NONE), kernels.get("observation", rr.NONE)
    P = _m(g["pose_est"] if poses is None else poses, (-1, 3)); Lm = _m(g["lm_est"] if lms is None else lms, (-1, 2))
    pf = np.zeros(len(P), dtype=bool); pf[np.asarray(g["fixed_poses"], dtype=np.int64)] = True
    lf = np.zeros(len(Lm), dtype=bool); lf[np.asarray(g["fixed_landmarks"], dtype=np.int64)] = True
    X = Exact(dict(Hpp_diag=len(P), Hll_diag=len(Lm), Hpp_off=len(g["pp_i"]), Hpl=len(g["pl_p"]), b_pose=len(P), b_lm=len(Lm)),
              k_pp[0] != "none" or k_pl[0] != "none")

    def quad(e, em, Js, Jms, W, kernel):
        """per edge: s, S_s, the weight and the blocks J_a^T W J_b, -J_a^T W e with their magnitudes (a <= b over the edge's vertices)"""
        Wm = mabs(W)
        s = mm(tr(col(e)), mm(W, col(e)))[0][0]; S_s = mm(tr(col(em)), mm(Wm, col(em)))[0][0]
        # what the error of s can be where it feeds a weight: to first order 2 |e|^T |W| de + roundings of |e|^T |W| |e|, de <= 14 u e~;
        # the second-order rest is below 34 u^2 e~^T |W| e~
        ea = col([abs(v) for v in e])
        S_s1 = 2 * mm(tr(col(em)), mm(Wm, ea))[0][0] + mm(tr(ea), mm(Wm, ea))[0][0] + 34 * U * S_s
        w, rho, S_w, S_rho = robust(kernel, s, S_s, S_s1)
        H = {}; b = []
        for a in range(len(Js)):
            b.append((fl(scal(mm(tr(Js[a]), mm(W, col(e))), -w)), fl(scal(mm(tr(Jms[a]), mm(Wm, col(em))), S_w))))
            for c in range(a, len(Js)):
                H[a, c] = (fl(scal(mm(tr(Js[a]), mm(W, Js[c])), w)), fl(scal(mm(tr(Jms[a]), mm(Wm, Jms[c])), S_w)))
        return s, S_s, rho, S_rho, H, b

    def count_chi(rho, S_rho):
        X.chi2 += rho; X.chi2_Sm += S_rho; X.chi2_n += 1; X.chi2_terms.append(rho); X.chi2_tags.append(None)

    Zpp = _m(g["pp_z"], (-1, 3)); Wpp = np.asarray(g["pp_info"], dtype=np.float64).reshape(-1, 3, 3)
    for k, (i, j) in enumerate(zip(g["pp_i"], g["pp_j"])):
        i, j = int(i), int(j)
        e = err_pp(P[i], P[j], Zpp[k]); em, Am, Bm = mag_pp(P[i], P[j], Zpp[k]); A, B = jac_pp(P[i], P[j], Zpp[k])
        s, S_s, rho, S_rho, H, b = quad(e, em, (A, B), (Am, Bm), _m(Wpp[k], (3, 3)), k_pp)
        X.s_pp.append(s); X.S_s_pp.append(float(S_s))
        if pf[i] and pf[j]:
            continue
        count_chi(rho, S_rho)
        if not pf[i]:
            X.add("Hpp_diag", i, *H[0, 0]); X.add("b_pose", i, *b[0])
        if not pf[j]:
            X.add("Hpp_diag", j, *H[1, 1]); X.add("b_pose", j, *b[1])
        if not pf[i] and not pf[j]:
            X.add("Hpp_off", k, *H[0, 1])
    Zpl = _m(g["pl_z"], (-1, 2)); Wpl = np.asarray(g["pl_info"], dtype=np.float64).reshape(-1, 2, 2)
    for k, (p, l) in enumerate(zip(g["pl_p"], g["pl_l"])):
        p, l = int(p), int(l)
        e = err_pl(P[p], Lm[l], Zpl[k]); em, Am, Bm = mag_pl(P[p], Lm[l], Zpl[k]); A, B = jac_pl(P[p], Lm[l])
        s, S_s, rho, S_rho, H, b = quad(e, em, (A, B), (Am, Bm), _m(Wpl[k], (2, 2)), k_pl)
        X.s_pl.append(s); X.S_s_pl.append(float(S_s))
        if pf[p] and lf[l]:
            continue
        count_chi(rho, S_rho)
        if not pf[p]:
            X.add("Hpp_diag", p, *H[0, 0]); X.add("b_pose", p, *b[0])
        if not lf[l]:
            X.add("Hll_diag", l, *H[1, 1]); X.add("b_lm", l, *b[1])
        if not pf[p] and not lf[l]:
            X.add("Hpl", k, *H[0, 1])
    return X.finish()


def magnitudes(g, poses=None, lms=None):
    """(S, n) per entry of the six arrays as Exact.S / Exact.n without a robust kernel, restated in float64 numpy for graphs that are too
    large for mpmath (S only scales a bound: its own rounding, 1e-15 relative, does not matter; test_tail_exact_cpu.py holds it to Exact.S)"""
    P = np.asarray(g["pose_est"] if poses is None else poses, dtype=np.float64).reshape(-1, 3); Lm = np.asarray(g["lm_est"] if lms is None else lms, dtype=np.float64).reshape(-1, 2)
    N, M = len(P), len(Lm)
    pf = np.zeros(N, dtype=bool); pf[np.asarray(g["fixed_poses"], dtype=np.int64)] = True
    lf = np.zeros(M, dtype=bool); lf[np.asarray(g["fixed_landmarks"], dtype=np.int64)] = True
    pp_i, pp_j = np.asarray(g["pp_i"], dtype=np.int64), np.asarray(g["pp_j"], dtype=np.int64)
    pl_p, pl_l = np.asarray(g["pl_p"], dtype=np.int64), np.asarray(g["pl_l"], dtype=np.int64)
    sizes = dict(Hpp_diag=N, Hll_diag=M, Hpp_off=len(pp_i), Hpl=len(pl_p), b_pose=N, b_lm=M)
    S = {k: np.zeros((sizes[k], WIDTH[k])) for k in ARRAYS}; n = {k: np.zeros((sizes[k], WIDTH[k]), dtype=np.int64) for k in ARRAYS}

    def put(name, rows, vals, mask):
        np.add.at(S[name], rows[mask], vals.reshape(len(rows), -1)[mask]); np.add.at(n[name], rows[mask], 1)
    # odometry edges (mag_pp)
    xi, xj, z = P[pp_i], P[pp_j], np.asarray(g["pp_z"], dtype=np.float64).reshape(-1, 3)
    W = np.abs(np.asarray(g["pp_info"], dtype=np.float64).reshape(-1, 3, 3))
    ci, si, cz, sz = np.abs(np.cos(xi[:, 2])), np.abs(np.sin(xi[:, 2])), np.abs(np.cos(z[:, 2])), np.abs(np.sin(z[:, 2]))
    ax, ay = np.abs(xj[:, 0]) + np.abs(xi[:, 0]), np.abs(xj[:, 1]) + np.abs(xi[:, 1])
    qx, qy = ci * ax + si * ay + np.abs(z[:, 0]), si * ax + ci * ay + np.abs(z[:, 1])
    e = np.stack([cz * qx + sz * qy, sz * qx + cz * qy, np.abs(xj[:, 2]) + np.abs(xi[:, 2]) + np.abs(z[:, 2])], axis=1)
    o, l = np.zeros_like(ci), np.ones_like(ci)
    Z = np.stack([np.stack([cz, sz, o], 1), np.stack([sz, cz, o], 1), np.stack([o, o, l], 1)], 1)
    Ji = np.stack([np.stack([ci, si, si * ax + ci * ay], 1), np.stack([si, ci, ci * ax + si * ay], 1), np.stack([o, o, l], 1)], 1)
    Jj = np.stack([np.stack([ci, si, o], 1), np.stack([si, ci, o], 1), np.stack([o, o, l], 1)], 1)
    A, B = Z @ Ji, Z @ Jj
    fi, fj = ~pf[pp_i], ~pf[pp_j]; k = np.arange(len(pp_i))
    AT, BT = A.transpose(0, 2, 1), B.transpose(0, 2, 1); We = (W @ e[:, :, None])
    put("Hpp_diag", pp_i, AT @ W @ A, fi); put("b_pose", pp_i, AT @ We, fi)
    put("Hpp_diag", pp_j, BT @ W @ B, fj); put("b_pose", pp_j, BT @ We, fj)
    put("Hpp_off", k, AT @ W @ B, fi & fj)
    # observation edges (mag_pl)
    xp, lm, z = P[pl_p], Lm[pl_l], np.asarray(g["pl_z"], dtype=np.float64).reshape(-1, 2)
    W = np.abs(np.asarray(g["pl_info"], dtype=np.float64).reshape(-1, 2, 2))
    c, s = np.abs(np.cos(xp[:, 2])), np.abs(np.sin(xp[:, 2])); px, py, lx_, ly = np.abs(xp[:, 0]), np.abs(xp[:, 1]), np.abs(lm[:, 0]), np.abs(lm[:, 1])
    e = np.stack([c * lx_ + s * ly + c * px + s * py + np.abs(z[:, 0]), s * lx_ + c * ly + s * px + c * py + np.abs(z[:, 1])], axis=1)
    A = np.stack([np.stack([c, s, c * ly + c * py + s * lx_ + s * px], 1), np.stack([s, c, s * ly + s * py + c * lx_ + c * px], 1)], 1)
    B = np.stack([np.stack([c, s], 1), np.stack([s, c], 1)], 1)
    fp, fl = ~pf[pl_p], ~lf[pl_l]; k = np.arange(len(pl_p))
    AT, BT = A.transpose(0, 2, 1), B.transpose(0, 2, 1); We = (W @ e[:, :, None])
    put("Hpp_diag", pl_p, AT @ W @ A, fp); put("b_pose", pl_p, AT @ We, fp)
    put("Hll_diag", pl_l, BT @ W @ B, fl); put("b_lm", pl_l, BT @ We, fl)
    put("Hpl", k, AT @ W @ B, fp & fl)
    return {k: v.reshape(-1) for k, v in S.items()}, {k: v.reshape(-1) for k, v in n.items()}


# ---- the checks
def _err(got, exact):
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    assert len(got) == len(exact), (len(got), len(exact))
    return np.array([float(abs(mpf(float(a)) - b)) for a, b in zip(got, exact)])


def _ratio(err, S):
    """err / (u S); an entry with S = 0 (nothing is summed into it) must be exactly zero"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(S > 0, err / (U * S), np.where(err == 0, 0.0, np.inf))


def check(X, blocks, chi2=None, s_pp=None, s_pl=None, tag=""):
    """asserts the bound on every entry of the six arrays (blocks = None: there is no export, as on a grown plan), on the chi2 total and on
    the per-edge s; returns the worst err / (u S) per array"""
    worst = {}
    for k in ARRAYS if blocks is not None else ():
        r = _ratio(_err(blocks[k], X.val[k]), X.S[k]); c = X.bound(k)
        worst[k] = float(r.max()) if len(r) else 0.0
        bad = np.flatnonzero(r > c)
        assert not len(bad), (tag, k, "entry", int(bad[0]) // WIDTH[k], int(bad[0]) % WIDTH[k], "err / (u S)", float(r[bad[0]]), "C", float(c[bad[0]]), "n", int(X.n[k][bad[0]]))
    if chi2 is not None:
        r = float(_ratio(_err([chi2], [X.chi2]), np.array([X.chi2_S]))[0]); worst["chi2"] = r
        assert r <= X.chi2_bound(), (tag, "chi2", r, float(X.chi2_bound()))
    for name, got, ex, S in (("s_pp", s_pp, X.s_pp, X.S_s_pp), ("s_pl", s_pl, X.s_pl, X.S_s_pl)):
        if got is not None:
            r = _ratio(_err(got, ex), np.asarray(S)); worst[name] = float(r.max()) if len(r) else 0.0
            c = 2.0 * (X.L_s_pl + 1.0) if name == "s_pl" and X.L_s_pl is not None else np.full(len(r), float(C(1)))
            bad = np.flatnonzero(r > c)
            assert not len(bad), (tag, name, "edge", int(bad[0]), "err / (u S)", float(r[bad[0]]), "C", float(c[bad[0]]))
    return worst


def check_can_fail(X, blocks, chi2=None, tag="", side=None):
    """the two-sided half: in every array the entry with the largest S gets one contributing edge's term (its largest) times (1 + 1e-9) in the
    reference, and `blocks` must then violate the bound there.  Where cancellation makes 2 C u S of that entry exceed 1e-9 |term| no fp64
    evaluation can tell the two references apart (kilometre coordinates: S of a theta-theta entry is 1e8 times the entry); the check then moves
    to the entry with the largest S at which it can, and says so in what it returns: {array: (flat index, perturbed err / (u S), C, moved)},
    None for an array (or for chi2, one number) in which 1e-9 of a term can show nowhere — the callers assert where that is allowed.
    side: the tag of a side pass ("polar", "prior"): the perturbed term is then one of that pass's own, and only arrays that hold such terms
    are reported."""
    out = {}
    for k in ARRAYS:
        mine = {idx: [t for t, g in zip(ts, X.tags[k][idx]) if side is None or g == side] for idx, ts in X.terms[k].items()}
        mine = {idx: ts for idx, ts in mine.items() if ts}
        if not mine:
            continue
        c = X.bound(k)
        big = np.zeros(len(X.S[k]))
        for idx, ts in mine.items():
            big[idx] = float(max(abs(t) for t in ts))
        can = REL * big > 2 * c * U * X.S[k]
        if not can.any():
            out[k] = None; continue
        first = int(np.argmax(X.S[k])); idx = first if can[first] else int(np.argmax(np.where(can, X.S[k], -1.0)))
        t = max(mine[idx], key=abs)
        got = mpf(float(np.asarray(blocks[k], dtype=np.float64).reshape(-1)[idx]))
        r = float(abs(got - (X.val[k][idx] + REL * t))) / (U * X.S[k][idx])
        assert r > c[idx], (tag, k, idx, "a term off by 1e-9 stays inside the bound", r, float(c[idx]))
        out[k] = (idx, r, float(c[idx]), idx != first)
    mine = [t for t, g in zip(X.chi2_terms, X.chi2_tags) if side is None or g == side]
    if chi2 is not None and mine:
        t = max(mine, key=abs); c = float(X.chi2_bound())
        if REL * float(abs(t)) > 2 * c * U * X.chi2_S:
            r = float(abs(mpf(float(chi2)) - (X.chi2 + REL * t))) / (U * X.chi2_S)
            assert r > c, (tag, "chi2", "a term off by 1e-9 stays inside the bound", r, c)
            out["chi2"] = (0, r, c, False)
        else:
            out["chi2"] = None
    return out


def assert_two_sided(moved, far, robust=False, tag=""):
    """where check_can_fail must have found a place: somewhere in each of the four H arrays, always; in H_ll, H_pl and H_pp_off at their
    largest S, and somewhere in b_pose and b_lm, unless the graph lies at kilometre coordinates (u S of a residual is then 1e-9 of it and
    more) or has a robust kernel (an edge's own s leaves its weight, and with it every term of b, less determined than 1e-9)"""
    for k in ("Hpp_diag", "Hll_diag", "Hpl", "Hpp_off"):
        assert moved[k] is not None, (tag, k)
    if not far and not robust:
        assert all(moved[k] is not None for k in ARRAYS), (tag, moved)
        assert not any(moved[k][3] for k in ("Hll_diag", "Hpl", "Hpp_off")), (tag, moved)
