"""The exact covariance-gated association (TEST-ONLY; mpmath, 60 digits) and the bounds its device paths are held to: per query and candidate
the exact Mahalanobis distance d2 with a bound B, per query the set of admissible answers.

Written from include/graphslam.h ("covariance-gated association") — not from the kernels:
    z = the A0 CoG-frame XY (frontend_exact_ref),  w = R(theta) z,  g = w + t,  r2 = zx^2 + zy^2,  wp = (-wy, wx)
    Q = (sr^2 / r2) w w^T + sb^2 wp wp^T + sxy^2 I,   P = G Sigma_p G^T, G = [I2 | wp] (Sigma_p: upper triangle),   A = Q + P once per query
    S = Sigma_j + A,  nu = l_j - g,  det = S00 S11 - S01^2,  d2 = (S11 nu0^2 - 2 S01 nu0 nu1 + S00 nu1^2) / det
    admissible: |type_j - type_i| < type_tol, sqrt(nu0^2 + nu1^2) < max_distance, det > 0, S00 > 0, d2 < gate_chi2
    index = the admissible j of smallest d2 (ties: lowest j), -1 / +inf when none; second_d2 = the smallest d2 of the others, +inf when none
    a query whose g is NaN (azimuth 0) or whose r is 0: -1.
Every input (poses, covariances, cones, sigmas, the gate) is the fp64 number the handle is given, taken exactly.

THE BOUND.  u = 2^-53.  Every quantity is carried as (exact value, e) with |device - exact| <= 2 e to first order: e collects u |result| for
every fp64 operation the header's formula needs (sqrt and division correctly rounded; cos / sin of the heading 4 u, as frontend_exact_ref
counts the device's sincos) and the operands' e through the derivative; the total is doubled at the end (second order, and an ulp of a
result is 2 u of it — the C(n) = 2 (L + n) of the other references).  One line per step, in the order the formula is written:
    zx, zy            frontend_exact_ref's A0 bound                                     e = Bz  (already a full bound: doubled again, harmless)
    c, s              sincos(theta)                                                     e = 4 u |c|, 4 u |s|
    wx = zx c - zy s  two products 1 each, subtraction 1                                e = |c| e_zx + |zx| e_c + u |zx c| + (same for zy s) + u |wx|
    gx = wx + tx      addition 1                                                        e = e_wx + u |gx|                      (wy, gy likewise)
    r2 = zx^2 + zy^2  squares 1, addition 1                                             e = 2 |zx| e_zx + u zx^2 + 2 |zy| e_zy + u zy^2 + u r2
    k  = sr^2 / r2    square 1, division 1                                              e = u sr^2 / r2 + k e_r2 / r2 + u k
    sb2, sx2          squares 1                                                         e = u sb2, u sx2
    Q00 = k wx wx + sb2 wy wy + sx2      products 2 + 2, additions 2                    by the product and sum rules below
    Q01 = k wx wy - sb2 wx wy            products 2 + 2, subtraction 1
    Q11 = k wy wy + sb2 wx wx + sx2
    P00 = a + 2 c13 ux + f ux ux,  P01 = b + c13 uy + c23 ux + f ux uy,  P11 = d + 2 c23 uy + f uy uy      u = wp, Sigma_p entries exact
    A   = Q + P       addition 1 each (none without a pose covariance)
    S   = Sigma_j + A addition 1 each, Sigma_j exact
    nu0 = lx - gx     subtraction 1                                                     e = e_gx + u |nu0|
    eu  = sqrt(nu0^2 + nu1^2)            squares 1, addition 1, sqrt 1                  e = (|nu0| e_nu0 + |nu1| e_nu1) / eu + 5/2 u eu  -> the Euclidean band
    det = S00 S11 - S01^2                products 1, subtraction 1                      e = |S11| e_S00 + |S00| e_S11 + 2 |S01| e_S01 + u (|S00 S11| + S01^2) + u |det|
                                         THE CANCELLATION: relative to det this is (|S00 S11| + S01^2) / det u and the S errors over det
    num = S11 nu0 nu0 - 2 S01 nu0 nu1 + S00 nu1 nu1      products 2 each (2 S01 exact), subtraction 1, addition 1
    d2  = num / det                      division 1                                     e = (e_num + |d2| e_det) / (|det| - 2 e_det) + u |d2|
    product rule   e(a b) = |a| e_b + |b| e_a + u |a b|;   sum rule   e(a + b) = e_a + e_b + u |a + b|
    B = 2 e_d2 (and the bands of the other tests are 2 e of eu, det, S00).
REFUSALS (assertions, as the other references do where "first order" ends): a candidate that passes the type and the Euclidean test within the
band and whose det is not surely <= 0 must have 2 e_det <= 1e-6 |det|, and B <= 1e-6 max(d2, 1e-9 gate_chi2); the Euclidean band must
be below 1e-9 max_distance.  Nothing here is fitted to a device output.

ADMISSIBLE ANSWERS.  A candidate is SURELY admissible when every test holds with its band to spare, POSSIBLY admissible when it holds within
the band.  The index must be a possibly-admissible j whose interval [d2 - B, d2 + B] reaches below the smallest upper end d2 + B over the
surely-admissible ones; -1 is allowed iff no candidate is surely admissible; out_d2 within B of that index's exact d2 (+inf for -1).  A query
is AMBIGUOUS when that set holds more than one answer.  out_second_d2 is checked on unambiguous queries: the same rule over the OTHER
candidates — within its bound of a possibly-admissible other whose interval reaches below the smallest upper end of the surely-admissible
others, +inf allowed iff no other is surely admissible.
Candidates are screened in fp64 (type test exact for the integer types used; Euclidean distance from the rounded g, error far below the
1e-6 relative margin taken) and only those within the margin of max_distance go to mpmath: the rest fail the Euclidean test surely."""
import numpy as np

import frontend_exact_ref as fx
import lin_exact_ref as lx

MP, mpf, U = lx.MP, lx.mpf, lx.U
INF = float("inf")
DEFAULTS = dict(gate_chi2=5.991464547107979, max_distance=3.0, type_tol=1e-4, sigma_range=0.3, sigma_bearing=0.02, sigma_xy=0.05)


class E:
    """(exact value, first-order error) of a device quantity; the rules of the module docstring"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0):
        self.v = v if isinstance(v, mpf) else mpf(float(v)); self.e = mpf(e)

    def __add__(self, o):
        o = o if isinstance(o, E) else E(o); v = self.v + o.v
        return E(v, self.e + o.e + U * abs(v))

    def __sub__(self, o):
        o = o if isinstance(o, E) else E(o); v = self.v - o.v
        return E(v, self.e + o.e + U * abs(v))

    def __mul__(self, o):
        o = o if isinstance(o, E) else E(o); v = self.v * o.v
        return E(v, abs(self.v) * o.e + abs(o.v) * self.e + U * abs(v))

    def twice(self):
        return E(2 * self.v, 2 * self.e)                       # exact in fp64

    def neg(self):
        return E(-self.v, self.e)


def params_of(**kw):
    p = dict(DEFAULTS); p.update(kw)
    return p


class Query:
    """the query's side of one observation: g, A = Q + P as E triples; valid False for a NaN query or r == 0"""

    def __init__(self, R, i, pose, pc, p):
        self.valid = not R.nan[i]
        if not self.valid:
            return
        zx = E(mpf(R.z_hi[i, 0]) + mpf(R.z_lo[i, 0]), mpf(R.Bz[i, 0])); zy = E(mpf(R.z_hi[i, 1]) + mpf(R.z_lo[i, 1]), mpf(R.Bz[i, 1]))
        th = mpf(float(pose[2])); cv, sv = MP.cos(th), MP.sin(th)
        c = E(cv, 4 * U * abs(cv)); s = E(sv, 4 * U * abs(sv))
        wx = zx * c - zy * s; wy = zx * s + zy * c
        self.gx = wx + E(pose[0]); self.gy = wy + E(pose[1])
        r2 = zx * zx + zy * zy
        if r2.v == 0:
            self.valid = False
            return
        assert r2.v > 1e-200, "r is tiny but not zero: the device's r2 may underflow"
        sr2 = E(p["sigma_range"]) * E(p["sigma_range"])
        kv = sr2.v / r2.v
        k = E(kv, sr2.e / r2.v + kv * r2.e / r2.v + U * kv)
        sb2 = E(p["sigma_bearing"]) * E(p["sigma_bearing"]); sx2 = E(p["sigma_xy"]) * E(p["sigma_xy"])
        a00 = ((k * wx) * wx + (sb2 * wy) * wy) + sx2
        a01 = (k * wx) * wy - (sb2 * wx) * wy
        a11 = ((k * wy) * wy + (sb2 * wx) * wx) + sx2
        if pc is not None:
            pc = np.asarray(pc, dtype=np.float64).reshape(9)
            a, b, c13, d, c23, f = (E(pc[t]) for t in (0, 1, 2, 4, 5, 8))
            ux, uy = wy.neg(), wx
            a00 = a00 + ((a + c13.twice() * ux) + (f * ux) * ux)
            a01 = a01 + (((b + c13 * uy) + c23 * ux) + (f * ux) * uy)
            a11 = a11 + ((d + c23.twice() * uy) + (f * uy) * uy)
        self.a00, self.a01, self.a11 = a00, a01, a11


class Cand:
    """one candidate of one query: exact d2, B, and whether it is surely / possibly admissible"""
    __slots__ = ("j", "d2", "B", "sure", "poss", "eu", "det")

    def __init__(self, q, j, l, cov, p):
        n0 = E(l[0]) - q.gx; n1 = E(l[1]) - q.gy
        eu2 = n0 * n0 + n1 * n1; euv = MP.sqrt(eu2.v)
        eu_e = (eu2.e / (2 * euv) if euv > 0 else MP.sqrt(eu2.e)) + U * euv
        md, gate = mpf(float(p["max_distance"])), mpf(float(p["gate_chi2"]))
        assert 2 * eu_e < 1e-9 * md, ("the Euclidean band is not small", float(eu_e))
        s00 = E(cov[0]) + q.a00; s01 = E(cov[1]) + q.a01; s11 = E(cov[3]) + q.a11
        det = s00 * s11 - s01 * s01
        self.j = j; self.eu = float(euv); self.det = float(det.v)
        e_sure = euv < md - 2 * eu_e; e_poss = euv <= md + 2 * eu_e
        self.d2 = None; self.B = None; self.sure = self.poss = False
        if not e_poss or det.v + 2 * det.e <= 0:                      # (det = 0 with e = 0, the all-zero case, lands here: surely not admissible)
            return
        assert 2 * det.e <= 1e-6 * abs(det.v), ("S is too close to singular for a first-order bound", j, float(det.v), float(det.e))
        num = ((s11 * n0) * n0 - (s01.twice() * n0) * n1) + (s00 * n1) * n1
        d2v = num.v / det.v
        d2e = (num.e + abs(d2v) * det.e) / (abs(det.v) - 2 * det.e) + U * abs(d2v)
        B = 2 * d2e
        self.d2 = d2v; self.B = B
        if s00.v + 2 * s00.e <= 0:
            return
        if d2v - B > gate:                                            # surely outside the gate: not a candidate
            return
        assert B <= 1e-6 * max(d2v, mpf(1e-9) * gate), ("the bound of d2 is not small against d2", j, float(d2v), float(B))
        self.poss = bool(d2v - B <= gate)                             # (the device's d2 < gate can hold only if the interval reaches below it)
        self.sure = bool(self.poss and e_sure and det.v > 2 * det.e and s00.v > 2 * s00.e and d2v + B < gate)


def _pick(cands, got_j=None):
    """the admissible answers over a list of candidates: (set of possibly-admissible j that may win, whether 'none' is allowed)"""
    sure = [c for c in cands if c.sure]
    if not sure:
        return [c for c in cands if c.poss], True
    top = min(c.d2 + c.B for c in sure)
    return [c for c in cands if c.poss and c.d2 - c.B <= top], False


class Ref:
    """the reference of one case: per query its candidates, the admissible winners and whether -1 is allowed"""

    def __init__(self, R, map_xy, map_ty, map_cov, pose_cov, params):
        self.R = R; self.p = p = params_of(**params); n = R.n
        map_xy = np.asarray(map_xy, dtype=np.float64).reshape(-1, 2); map_ty = np.asarray(map_ty, dtype=np.int64).reshape(-1); m = len(map_xy)
        map_cov = np.zeros((m, 4)) if map_cov is None else np.asarray(map_cov, dtype=np.float64).reshape(-1, 4)
        assert len(map_cov) == m and len(map_ty) == m
        self.map_xy, self.map_ty, self.map_cov = map_xy, map_ty, map_cov
        self.cands = [[] for _ in range(n)]; self.valid = np.zeros(n, dtype=bool); self.n_pairs = 0
        md = float(p["max_distance"])
        for i in range(n):
            pi = int(R.pose_of[i])
            q = Query(R, i, R.poses[pi], None if pose_cov is None else np.asarray(pose_cov, dtype=np.float64).reshape(-1, 9)[pi], p)
            self.valid[i] = q.valid
            if not q.valid or m == 0:
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                ok = np.abs(map_ty.astype(np.float64) - R.obs[i, 3]) < p["type_tol"]
                D = np.hypot(map_xy[:, 0] - R.g_hi[i, 0], map_xy[:, 1] - R.g_hi[i, 1])
                near = ok & (D < md * (1 + 1e-6) + 1e-9)
            for j in np.flatnonzero(near):
                self.cands[i].append(Cand(q, int(j), map_xy[j], map_cov[j], p)); self.n_pairs += 1
        self.win = [None] * n; self.none_ok = np.ones(n, dtype=bool)
        for i in range(n):
            self.win[i], self.none_ok[i] = _pick(self.cands[i])

    def ambiguous(self, i):
        return len(self.win[i]) + (1 if self.none_ok[i] else 0) > 1

    def n_ambiguous(self):
        return sum(self.ambiguous(i) for i in range(self.R.n))

    def unique_answer(self):
        """per query the one admissible index (-1: none), or -2 where the query is ambiguous"""
        out = np.full(self.R.n, -2, dtype=np.int64)
        for i in range(self.R.n):
            if not self.ambiguous(i):
                out[i] = self.win[i][0].j if self.win[i] else -1
        return out

    def failures(self, idx, d2, second):
        """[(query, what)] for every answer that is not admissible; also fills self.worst = (largest |d2 - exact| / B, the same for second_d2)"""
        idx = np.asarray(idx, dtype=np.int64).reshape(-1); d2 = np.asarray(d2, dtype=np.float64).reshape(-1); second = np.asarray(second, dtype=np.float64).reshape(-1)
        assert len(idx) == len(d2) == len(second) == self.R.n
        bad = []; w1 = w2 = 0.0
        for i in range(self.R.n):
            if idx[i] == -1:
                if not self.none_ok[i]:
                    bad.append((i, "-1 where a candidate is surely admissible"))
                elif not (d2[i] == INF and second[i] == INF):
                    bad.append((i, "-1 without +inf in d2 / second_d2"))
                continue
            hit = [c for c in self.win[i] if c.j == idx[i]]
            if not hit:
                bad.append((i, "index %d is not an admissible winner %s" % (idx[i], sorted(c.j for c in self.win[i]))))
                continue
            c = hit[0]; r = abs(mpf(float(d2[i])) - c.d2) / c.B if c.B > 0 else (mpf(0) if mpf(float(d2[i])) == c.d2 else mpf(INF))
            w1 = max(w1, float(r))
            if not r <= 1:
                bad.append((i, "d2 %.17g off the exact %.17g by %.3g B" % (d2[i], float(c.d2), float(r))))
                continue
            if self.ambiguous(i):
                continue
            others = [o for o in self.cands[i] if o.j != c.j]
            win2, none2 = _pick(others)
            if second[i] == INF:
                if not none2:
                    bad.append((i, "second_d2 +inf where another candidate is surely admissible"))
                continue
            rr = [abs(mpf(float(second[i])) - o.d2) / o.B if o.B > 0 else (mpf(0) if mpf(float(second[i])) == o.d2 else mpf(INF)) for o in win2]
            if not rr or not min(rr) <= 1:
                bad.append((i, "second_d2 %.17g is no admissible runner-up's d2 (%s)" % (second[i], [float(o.d2) for o in win2][:4])))
            else:
                w2 = max(w2, float(min(rr)))
        self.worst = (w1, w2)
        return bad

    def check(self, idx, d2, second, tag=""):
        bad = self.failures(idx, d2, second)
        if bad:
            raise AssertionError((tag, bad[0], "%d queries fail" % len(bad)))
        return self.worst


def make(case):
    """the reference of a case dict of assoc_nn_shapes (its A0 through frontend_exact_ref, which no query of a case may leave in the branch band)"""
    R = fx.Ref(case["obs"], case["poses"], case["pose_of"], case["lidar"])
    assert not R.band.any(), ("a query in A0's branch band", case.get("name"))
    return Ref(R, case["map_xy"], case["map_ty"], case["map_cov"], case["pose_cov"], case["params"])
