"""The exact map twins (TEST-ONLY; mpmath, 60 digits) and the bounds the device is held to.  Written from include/graphslam.h ("map twins"),
not from the kernels:
    pair of cones i != j, formed from a = min(i, j), b = max(i, j):   s2 = sigma_floor^2 (the fp64 product, formed once on the host)
    A = Sigma_a + s2 I,  B = Sigma_b + s2 I,  S = A + B,  nu = l_b - l_a,  det = S00 S11 - S01^2,
    d2 = (((S11 nu0) nu0 - ((2 S01) nu0) nu1) + (S00 nu1) nu1) / det
    admissible: equal types (require_same_type), sqrt(nu0^2 + nu1^2) < max_distance, det > 0, S00 > 0, d2 < gate_chi2 (positive tests)
    twin[i] = the admissible j of smallest d2 (ties: lowest j), -1 / +inf when none; second_d2; n_admissible
    twin pair (a, b): twin[a] == b and twin[b] == a (exclusive: n_admissible == 1 at both ends); keeper a:
    K = A S^-1 entry by entry, l+ = l_a + K nu, C+ = K B (three entries, 01 formed once); b dropped, order kept, remap, gs_dup_info.
Every input is the fp64 number given, taken exactly.

THE BOUND.  assoc_nn_ref's E pairs: every quantity is (exact value, e) with |device - exact| <= 2 e to first order — u |result| per fp64
operation, the operands' e through the derivative, B = 2 e.  A quotient q = a / b has e = (e_a + |q| e_b) / (|b| - 2 e_b) + u |q|.
REFUSALS (assertions, where first order ends): a pair that reaches the determinant must have 2 e_det <= 1e-6 |det|, and one that reaches the
gate B <= 1e-6 max(d2, 1e-9 gate_chi2).

DECISIONS.  Every comparison that decides something — the Euclidean test, det > 0, S00 > 0, the gate, which admissible cone is nearest — must
hold or fail with its band (2 e of either side) to spare.  A scene in which one falls inside its band is REJECTED (the exception below), not
excused: the shapes are built so that none is.  One tie is certified instead of rejected: two candidates of a cone whose S entries are equal
and whose nu are equal or opposite give equal bits under the formula above, whatever the rounding; the lowest index wins it.
Given the decisions, twin, n_admissible, remap, the counters, every untouched cone and the keeper's type are held BIT FOR BIT; d2, second_d2,
l+ and C+ within B.

Pairs are screened in fp64 (Euclidean distance with a 1e-6 relative margin, error far below it; a sweep along x): the rest fail the Euclidean
test surely.
replay(): the same rule in float64 (python floats: one rounding per operation, no contraction) for the CPU tests."""
import math

import numpy as np

import assoc_nn_ref as nr

MP, mpf, U, E = nr.MP, nr.mpf, nr.U, nr.E
INF = float("inf")


class Rejected(Exception):
    """a deciding comparison of the scene lies inside its error band"""


def _div(a, b):
    q = a.v / b.v
    return E(q, (a.e + abs(q) * b.e) / (abs(b.v) - 2 * b.e) + U * abs(q))


def _decide(lhs, band, rhs, what):
    """lhs < rhs with the band to spare: True / False, or Rejected"""
    if lhs + band < rhs:
        return True
    if lhs - band > rhs or (band == 0 and lhs >= rhs):
        return False
    raise Rejected(what)


def _near_pairs(xy, ty, p):
    """[(a, b)], a < b, ascending, that may pass the type and the Euclidean test; NaN cones are in none.  A sweep along x: a cone is held
    against those whose x lies within the margin above its own, so a large map costs its near pairs, not all of them"""
    md = float(p["max_distance"]) * (1 + 1e-6) + 1e-9
    fin = np.flatnonzero(np.isfinite(xy).all(axis=1))
    order = fin[np.argsort(xy[fin, 0], kind="stable")]; xs = xy[order, 0]; ys = xy[order, 1]; ts = ty[order]
    hi = np.searchsorted(xs, xs + md, side="right")
    out = []
    for i in range(len(order)):
        if hi[i] - i < 2:
            continue
        ok = np.hypot(xs[i + 1:hi[i]] - xs[i], ys[i + 1:hi[i]] - ys[i]) < md
        if p["require_same_type"]:
            ok &= ts[i + 1:hi[i]] == ts[i]
        for k in np.flatnonzero(ok):
            a, b = int(order[i]), int(order[i + 1 + k])
            out.append((min(a, b), max(a, b)))
    return sorted(out)


class Pair:
    """one pair (a, b), a < b: its exact quantities as E, whether it is admissible (decided, or Rejected), its d2 and B"""

    def __init__(self, a, b, xy, cov, p):
        self.a, self.b = a, b
        s2 = E(float(p["sigma_floor"]) * float(p["sigma_floor"]))
        ca, cb = cov[a], cov[b]
        self.A = (E(ca[0]) + s2, E(ca[1]), E(ca[3]) + s2); self.B = (E(cb[0]) + s2, E(cb[1]), E(cb[3]) + s2)
        self.S = tuple(x + y for x, y in zip(self.A, self.B))
        self.n0 = E(xy[b, 0]) - E(xy[a, 0]); self.n1 = E(xy[b, 1]) - E(xy[a, 1])
        self.key = (tuple(s.v for s in self.S), abs(self.n0.v), abs(self.n1.v), (self.n0.v * self.n1.v > 0) - (self.n0.v * self.n1.v < 0))
        s00, s01, s11 = self.S; n0, n1 = self.n0, self.n1
        eu2 = n0 * n0 + n1 * n1; eu = MP.sqrt(eu2.v)
        eu_e = (eu2.e / (2 * eu) if eu > 0 else MP.sqrt(eu2.e)) + U * eu
        self.adm = False; self.d2 = None
        tag = "pair (%d, %d): " % (a, b)
        if not _decide(eu, 2 * eu_e, mpf(float(p["max_distance"])), tag + "the Euclidean test"):
            return
        self.det = det = s00 * s11 - s01 * s01
        if not _decide(mpf(0), 2 * det.e, det.v, tag + "det > 0"):
            return
        assert 2 * det.e <= 1e-6 * abs(det.v), (tag + "S is too close to singular for a first-order bound", float(det.v), float(det.e))
        if not _decide(mpf(0), 2 * s00.e, s00.v, tag + "S00 > 0"):
            return
        num = ((s11 * n0) * n0 - (s01.twice() * n0) * n1) + (s00 * n1) * n1
        self.d2 = _div(num, det); self.Bd = 2 * self.d2.e
        gate = mpf(float(p["gate_chi2"]))
        if self.d2.v - self.Bd > gate:
            return
        assert self.Bd <= 1e-6 * max(self.d2.v, mpf(1e-9) * gate), (tag + "the bound of d2 is not small against d2", float(self.d2.v), float(self.Bd))
        self.adm = _decide(self.d2.v, self.Bd, gate, tag + "the gate")

    def fused(self, xy):
        """[x+, y+, C00+, C01+, C11+] as E"""
        a00, a01, a11 = self.A; b00, b01, b11 = self.B; s00, s01, s11 = self.S; det = self.det; n0, n1 = self.n0, self.n1
        k00 = _div(a00 * s11 - a01 * s01, det); k01 = _div(a01 * s00 - a00 * s01, det)
        k10 = _div(a01 * s11 - a11 * s01, det); k11 = _div(a11 * s00 - a01 * s01, det)
        x = E(xy[self.a, 0]) + (k00 * n0 + k01 * n1); y = E(xy[self.a, 1]) + (k10 * n0 + k11 * n1)
        return [x, y, k00 * b00 + k01 * b01, k00 * b01 + k01 * b11, k10 * b01 + k11 * b11]


class Ref:
    """the reference of one map: decided twins (or Rejected), the consolidated map with bounds"""

    def __init__(self, xy, ty, cov, params):
        self.xy = xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2); self.ty = ty = np.asarray(ty, dtype=np.int32).reshape(-1); n = self.n = len(xy)
        self.has_cov = cov is not None
        self.cov = cov = np.zeros((n, 4)) if cov is None else np.asarray(cov, dtype=np.float64).reshape(-1, 4)
        self.p = p = dict(params)
        self.pairs = {}
        cands = [[] for _ in range(n)]
        for a, b in _near_pairs(xy, ty, p):
            pr = Pair(a, b, xy, cov, p); self.pairs[(a, b)] = pr
            if pr.adm:
                cands[a].append((b, pr)); cands[b].append((a, pr))
        self.n_values = sum(1 for pr in self.pairs.values() if pr.d2 is not None)
        self.twin = np.full(n, -1, dtype=np.int32); self.nadm = np.zeros(n, dtype=np.int32)
        self.d2 = [None] * n; self.second = [None] * n                       # (E value, bound) or None for +inf
        for i in range(n):
            c = sorted(cands[i], key=lambda t: (t[1].d2.v, t[0])); self.nadm[i] = len(c)
            if not c:
                continue
            j0, p0 = c[0]
            for j, pr in c[1:]:
                if pr.d2.v - pr.Bd > p0.d2.v + p0.Bd:
                    break
                if pr.key != p0.key:                                           # not the certified tie: the arg-min is inside its band
                    raise Rejected("cone %d: candidates %d and %d are not separated" % (i, j0, j))
            self.twin[i] = j0; self.d2[i] = (p0.d2.v, p0.Bd)
            if len(c) > 1:
                v = c[1][1].d2.v; bb = max(pr.Bd for _, pr in c[1:] if pr.d2.v - pr.Bd <= v + c[1][1].Bd)
                self.second[i] = (v, bb)
        ex = bool(p["exclusive"])
        self.twin_pairs = [(a, int(self.twin[a])) for a in range(n)
                           if self.twin[a] > a and self.twin[self.twin[a]] == a and (not ex or (self.nadm[a] == 1 and self.nadm[self.twin[a]] == 1))]
        drop = {b: a for a, b in self.twin_pairs}
        self.remap = np.zeros(n, dtype=np.int32); k = 0
        for i in range(n):
            if i not in drop:
                self.remap[i] = k; k += 1
        for b, a in drop.items():
            self.remap[b] = self.remap[a]
        self.n_out = k
        self.info = dict(n_in=n, n_out=k, n_pairs=len(self.twin_pairs), n_ambiguous=int((self.nadm > 1).sum()))
        self.fused = {a: self.pairs[(a, b)].fused(xy) for a, b in self.twin_pairs}
        self.worst = 0.0

    def _within(self, got, v, B):
        d = abs(mpf(float(got)) - v)
        r = float(d / B) if B > 0 else (0.0 if d == 0 else INF)
        self.worst = max(self.worst, r)
        return r <= 1

    def twins_failures(self, twin, d2, second, nadm):
        twin = np.asarray(twin); d2 = np.asarray(d2, dtype=np.float64); second = np.asarray(second, dtype=np.float64); nadm = np.asarray(nadm)
        assert len(twin) == len(d2) == len(second) == len(nadm) == self.n
        bad = []
        for i in range(self.n):
            if twin[i] != self.twin[i]:
                bad.append((i, "twin %d, not %d" % (twin[i], self.twin[i])))
            if nadm[i] != self.nadm[i]:
                bad.append((i, "n_admissible %d, not %d" % (nadm[i], self.nadm[i])))
            for got, want, what in ((d2[i], self.d2[i], "d2"), (second[i], self.second[i], "second_d2")):
                if want is None:
                    if got != INF:
                        bad.append((i, "%s %r where +inf is due" % (what, got)))
                elif not self._within(got, want[0], want[1]):
                    bad.append((i, "%s %.17g off the exact %.17g" % (what, got, float(want[0]))))
        return bad

    def merge_failures(self, xy, ty, cov, remap, info):
        xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2); ty = np.asarray(ty); remap = np.asarray(remap)
        bad = []
        got_info = {k: int(info[k]) for k in ("n_in", "n_out", "n_pairs", "n_ambiguous")}
        if got_info != self.info:
            bad.append((-1, "info %r, not %r" % (got_info, self.info)))
        if len(remap) != self.n or not np.array_equal(remap, self.remap):
            bad.append((-1, "remap differs" + ("" if len(remap) != self.n else " first at %d" % int(np.flatnonzero(remap != self.remap)[0]))))
        if len(xy) != self.n_out or len(ty) != self.n_out or (self.has_cov and (cov is None or len(cov) != self.n_out)):
            return bad + [(-1, "the consolidated map has %d cones, not %d" % (len(xy), self.n_out))]
        cv = None if not self.has_cov else np.asarray(cov, dtype=np.float64).reshape(-1, 4)
        dropped = {b for _, b in self.twin_pairs}
        for i in range(self.n):
            if i in dropped:
                continue
            k = int(self.remap[i])
            if ty[k] != self.ty[i]:
                bad.append((i, "type %d, not %d" % (ty[k], self.ty[i])))
            if i not in self.fused:
                if xy[k].tobytes() != self.xy[i].tobytes() or (cv is not None and cv[k].tobytes() != self.cov[i].tobytes()):
                    bad.append((i, "an untouched cone changed bits"))
                continue
            f = self.fused[i]
            got = [xy[k, 0], xy[k, 1]] + ([cv[k, 0], cv[k, 1], cv[k, 3]] if cv is not None else [])
            for g, w, what in zip(got, f, ("x+", "y+", "C00+", "C01+", "C11+")):
                if not self._within(g, w.v, 2 * w.e):
                    bad.append((i, "%s %.17g off the exact %.17g (B %.3g)" % (what, g, float(w.v), float(2 * w.e))))
            if cv is not None and cv[k, 1].tobytes() != cv[k, 2].tobytes():
                bad.append((i, "C+ is not bitwise symmetric"))
        return bad


def make(sc, params):
    return Ref(sc["xy"], sc["ty"], sc["cov"], params)


# ---- the float64 replay
def _pair64(a, b, xy, cov, p, s2):
    """(admissible, d2, (A, B, S, det, n0, n1)) of a < b in float64, the header's order"""
    A = (cov[a][0] + s2, cov[a][1], cov[a][3] + s2); B = (cov[b][0] + s2, cov[b][1], cov[b][3] + s2)
    s00, s01, s11 = A[0] + B[0], A[1] + B[1], A[2] + B[2]
    n0 = xy[b][0] - xy[a][0]; n1 = xy[b][1] - xy[a][1]
    r2 = n0 * n0 + n1 * n1
    if not (r2 == r2 and math.sqrt(r2) < p["max_distance"]):
        return False, INF, None
    det = s00 * s11 - s01 * s01
    if not det > 0.0:
        return False, INF, None
    d2 = (((s11 * n0) * n0 - ((2.0 * s01) * n0) * n1) + (s00 * n1) * n1) / det
    return bool(s00 > 0.0 and d2 < p["gate_chi2"]), d2, (A, B, (s00, s01, s11), det, n0, n1)


def replay(xy, ty, cov, params):
    """the rule in float64: dict(twin, d2, second, nadm, xy, ty, cov (None without an input cov), remap, info)"""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2); ty = np.asarray(ty, dtype=np.int32).reshape(-1); n = len(xy); p = dict(params)
    has_cov = cov is not None
    cov = np.zeros((n, 4)) if cov is None else np.asarray(cov, dtype=np.float64).reshape(-1, 4)
    X = xy.tolist(); Cv = cov.tolist(); s2 = float(p["sigma_floor"]) * float(p["sigma_floor"])
    twin = np.full(n, -1, dtype=np.int32); d2 = np.full(n, INF); second = np.full(n, INF); nadm = np.zeros(n, dtype=np.int32)
    near = [[] for _ in range(n)]; terms = {}
    for a, b in _near_pairs(xy, ty, p):
        ok, v, t = _pair64(a, b, X, Cv, p, s2)
        if ok:
            near[a].append((b, v)); near[b].append((a, v)); terms[(a, b)] = t
    for i in range(n):
        for j, v in sorted(near[i]):
            nadm[i] += 1
            if v < d2[i]:
                second[i] = d2[i]; d2[i] = v; twin[i] = j
            elif v < second[i]:
                second[i] = v
    ex = bool(p["exclusive"])
    pairs = [(a, int(twin[a])) for a in range(n) if twin[a] > a and twin[twin[a]] == a and (not ex or (nadm[a] == 1 and nadm[twin[a]] == 1))]
    drop = {b for _, b in pairs}; keep = [i for i in range(n) if i not in drop]
    remap = np.zeros(n, dtype=np.int32); remap[keep] = np.arange(len(keep))
    oxy = xy[keep].copy(); oty = ty[keep].copy(); ocv = cov[keep].copy()
    for a, b in pairs:
        remap[b] = remap[a]
        A, B, S, det, n0, n1 = terms[(a, b)]; s00, s01, s11 = S
        k00 = ((A[0] * s11) - (A[1] * s01)) / det; k01 = ((A[1] * s00) - (A[0] * s01)) / det
        k10 = ((A[1] * s11) - (A[2] * s01)) / det; k11 = ((A[2] * s00) - (A[1] * s01)) / det
        k = remap[a]
        oxy[k] = (X[a][0] + ((k00 * n0) + (k01 * n1)), X[a][1] + ((k10 * n0) + (k11 * n1)))
        f01 = (k00 * B[1]) + (k01 * B[2])
        ocv[k] = ((k00 * B[0]) + (k01 * B[1]), f01, f01, (k10 * B[1]) + (k11 * B[2]))
    info = dict(n_in=n, n_out=len(keep), n_pairs=len(pairs), n_ambiguous=int((nadm > 1).sum()))
    return dict(twin=twin, d2=d2, second=second, nadm=nadm, xy=oxy, ty=oty, cov=ocv if has_cov else None, remap=remap, info=info, pairs=pairs)
