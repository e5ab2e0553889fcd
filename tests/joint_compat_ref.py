"""The joint compatibility test of a frame's hypothesis (TEST-ONLY; mpmath, 60 digits), written from include/graphslam.h ("joint compatibility")
— not from the kernel — and the bounds the device is held to.

    pair (i, j = index[i] != -1):  D = Sigma_j + Q (Q: the covariance-gated association's, WITHOUT a pose covariance),  nu = l_j - g,
        a = nu^T D^-1 nu,  y = D^-1 nu,  c = (y0, y1, wp . y),  M = G^T D^-1 G with G = [I2 | wp], wp = (-w_y, w_x)
        in K iff the query is valid, 0 <= j < n_map, det D > 0, D00 > 0; otherwise untestable
    J(K) = a - c^T delta,  delta = Sigma_p (I + M Sigma_p)^-1 c  (a, c, M summed over K; Sigma_p = 0: delta = 0, J = a)
    while K is not empty and not J(K) < gate[|K|]: remove the pair of smallest J(K \\ {r}), ties to the lowest observation
brute() is the same J as the dense nu^T (blockdiag(D) + G Sigma_p G^T)^-1 nu over the stacked pairs, for small frames.

THE BOUND B.  u = 2^-53.  Every device quantity is carried as assoc_nn_ref.E = (exact value, e) with |device - exact| <= 2 e to first order; e
collects u |result| per fp64 operation the header writes down and the operands' e through the derivative (product, sum and quotient rules of
assoc_nn_ref, whose Query supplies g and Q with their e).  In the header's order:
    per pair   D = Sigma_j + Q 1 each;  nu 1 each;  det 3;  a: nn_pair's count (8 and the division);  y0, y1: 3 and the division;
               c2 = wp_x y0 + wp_y y1: 3;  E00, E01, E11: a division each;  h0, h1: 3 each;  M22: 3        — 10 terms t_0 .. t_9
    sums       a term passes through at most 10 additions (4 inside its lane, from +0; 6 butterfly levels):
               e(S) = sum e(t_i) + 10 u sum |t_i|                     — per round, from the kept pairs alone: NO dependence on the round number
    leave-one-out   R = S - t_r, 1 each:   e(R) = e(S) + u |R|        (e(S) already holds e(t_r))
    solve      A = I + M P: 3 products, 2 additions, on the diagonal 1 more;  9 cofactors: 3 each;  detA: 5;  x_s: 5 and the division;
               delta_r: 5;  J = a - c . delta: 6          — about 120 operations, each entering through the rules, none counted twice
    B(K) = 2 e(J), B of delta_r = 2 e(delta_r).  For k pairs of comparable size this is u (10 + O(1)) sum |a_i| plus the pairs' own e, amplified by
    the cancellation in a - c . delta where Sigma_p explains most of a: B grows like k through the sums and NOT with the rounds.
Nothing here is fitted to a device output.  1000 B is the headroom a comparison needs to count as decided (second order, and the rules being
first order: the same factor as assign_opt_ref's).

DECIDED.  A frame is DECIDED when every pair's tests are sure (valid query; det and D00 beyond twice their e), and every comparison the
elimination made has margin: |J(K) - gate[|K|]| >= 1000 B(K) in every round, and in every removal the runner-up's J(K \\ {r}) exceeds the
winner's by at least 1000 (B_winner + B_runner-up).  Then the device must return the reference's kept set, counts, J within B and delta within
its B.  Whatever the frame, a result must be VALID: kept pairs a subset of the hypothesis' testable pairs, n_kept their number, n_kept +
n_dropped + n_untestable = the observations with index != -1, the reported J within B of the exact J of the REPORTED kept set (delta
likewise), and J < gate[n_kept] or n_kept == 0."""
import numpy as np

import assoc_nn_ref as nr
import frontend_exact_ref as fx

MP, mpf, U, E = nr.MP, nr.mpf, nr.U, nr.E
INF = float("inf")
FRAME_MAX = 256
HEADROOM = 1000


def ediv(a, b):
    """the quotient rule of assoc_nn_ref's d2"""
    v = a.v / b.v
    assert abs(b.v) > 4 * b.e, "a divisor is not surely away from zero"
    return E(v, (a.e + abs(v) * b.e) / (abs(b.v) - 2 * b.e) + U * abs(v))


def chi2_cdf(m, x):
    import mpmath
    return mpmath.gammainc(m, 0, mpmath.mpf(x) / 2, regularized=True)


class Pair:
    """one pair of a hypothesis: its ten terms as E (t), or untestable; sure = every test it went through holds beyond its band"""

    def __init__(self, R, i, pose, j, map_xy, map_cov, p):
        self.i = i; self.j = j; self.t = None; self.testable = False; self.sure = True
        q = nr.Query(R, i, pose, None, p)
        if not (q.valid and 0 <= j < len(map_xy)):
            return
        zx = E(mpf(R.z_hi[i, 0]) + mpf(R.z_lo[i, 0]), mpf(R.Bz[i, 0])); zy = E(mpf(R.z_hi[i, 1]) + mpf(R.z_lo[i, 1]), mpf(R.Bz[i, 1]))
        th = mpf(float(pose[2])); cv, sv = MP.cos(th), MP.sin(th)
        c = E(cv, 4 * U * abs(cv)); s = E(sv, 4 * U * abs(sv))
        ux = (zx * s + zy * c).neg(); uy = zx * c - zy * s                    # wp = (-w_y, w_x)
        l = map_xy[j]; cov = np.zeros(4) if map_cov is None else map_cov[j]
        n0 = E(l[0]) - q.gx; n1 = E(l[1]) - q.gy
        d00 = E(cov[0]) + q.a00; d01 = E(cov[1]) + q.a01; d11 = E(cov[3]) + q.a11
        det = d00 * d11 - d01 * d01
        self.det = det; self.d00 = d00
        if not (det.v > 0 and d00.v > 0):
            self.sure = det.v < -2 * det.e or d00.v < -2 * d00.e or (det.v == 0 and det.e == 0)
            return
        self.sure = det.v > 4 * det.e and d00.v > 2 * d00.e
        if not self.sure:
            return
        self.testable = True
        a = ediv(((d11 * n0) * n0 - (d01.twice() * n0) * n1) + (d00 * n1) * n1, det)
        y0 = ediv(d11 * n0 - d01 * n1, det); y1 = ediv(d00 * n1 - d01 * n0, det)
        e00 = ediv(d11, det); e01 = ediv(d01, det).neg(); e11 = ediv(d00, det)
        h0 = e00 * ux + e01 * uy; h1 = e01 * ux + e11 * uy
        self.t = [a, y0, y1, ux * y0 + uy * y1, e00, e01, h0, e11, h1, ux * h0 + uy * h1]
        self.nu = (n0.v, n1.v); self.D = (d00.v, d01.v, d11.v); self.wp = (ux.v, uy.v)


def sums(pairs):
    """the ten sums over `pairs` as E: e(S) = sum e(t) + 10 u sum |t|"""
    out = []
    for q in range(10):
        v = mpf(0); e = mpf(0); ab = mpf(0)
        for pr in pairs:
            v += pr.t[q].v; e += pr.t[q].e; ab += abs(pr.t[q].v)
        out.append(E(v, e + 10 * U * ab))
    return out


def without(S, pr):
    return [E(S[q].v - pr.t[q].v, S[q].e + U * abs(S[q].v - pr.t[q].v)) for q in range(10)]


def solve(S, P):
    """(J, [delta]) as E from the sums S and Sigma_p's upper triangle P (6 floats) or None — the header's operation order"""
    if P is None:
        return S[0], [E(0), E(0), E(0)]
    c = S[1:4]; m00, m01, m02, m11, m12, m22 = S[4:]
    p00, p01, p02, p11, p12, p22 = (E(x) for x in P)
    M = [[m00, m01, m02], [m01, m11, m12], [m02, m12, m22]]; Pm = [[p00, p01, p02], [p01, p11, p12], [p02, p12, p22]]
    A = [[(M[r][0] * Pm[0][s] + M[r][1] * Pm[1][s]) + M[r][2] * Pm[2][s] for s in range(3)] for r in range(3)]
    for r in range(3):
        A[r][r] = E(1) + A[r][r]
    C = [[None] * 3 for _ in range(3)]
    for r in range(3):
        for s in range(3):
            r1, r2 = (r + 1) % 3, (r + 2) % 3; s1, s2 = (s + 1) % 3, (s + 2) % 3      # the cyclic form of the cofactor: the header's nine lines
            C[r][s] = A[r1][s1] * A[r2][s2] - A[r1][s2] * A[r2][s1]
    det = (A[0][0] * C[0][0] + A[0][1] * C[0][1]) + A[0][2] * C[0][2]
    x = [ediv((C[0][s] * c[0] + C[1][s] * c[1]) + C[2][s] * c[2], det) for s in range(3)]
    dl = [(Pm[r][0] * x[0] + Pm[r][1] * x[1]) + Pm[r][2] * x[2] for r in range(3)]
    return S[0] - ((c[0] * dl[0] + c[1] * dl[1]) + c[2] * dl[2]), dl


def upper(pc):
    if pc is None:
        return None
    pc = np.asarray(pc, dtype=np.float64).reshape(9)
    return [float(pc[t]) for t in (0, 1, 2, 4, 5, 8)]


class FrameRef:
    """one frame: members = observation numbers of R (a frontend_exact_ref.Ref) in the frame's order, hyp = the hypothesis in that order,
    pose = the frame's pose (x, y, theta), pose_cov = its 9 numbers or None, gate = the table (257 floats), p = assoc_nn_ref.params_of(...)"""

    def __init__(self, R, members, hyp, pose, pose_cov, map_xy, map_cov, gate, p, cache=None):
        self.k = len(members); self.hyp = [int(j) for j in hyp]; self.gate = [float(x) for x in gate]; self.P = upper(pose_cov)
        map_xy = np.asarray(map_xy, dtype=np.float64).reshape(-1, 2)
        map_cov = None if map_cov is None else np.asarray(map_cov, dtype=np.float64).reshape(-1, 4)
        self.pairs = {}; self.n_untestable = 0; self.sure = True
        for a, (i, j) in enumerate(zip(members, self.hyp)):
            if j == -1:
                continue
            pr = cache.get((int(i), j)) if cache is not None else None         # (a pair does not depend on the frame it is in)
            if pr is None:
                pr = Pair(R, int(i), pose, j, map_xy, map_cov, p)
                if cache is not None:
                    cache[(int(i), j)] = pr
            self.sure &= pr.sure
            if pr.testable:
                self.pairs[a] = pr
            else:
                self.n_untestable += 1
        self.n_named = sum(j != -1 for j in self.hyp)
        self.eliminated = False

    def J_of(self, kept):
        """(exact J, B, [exact delta], [B of delta]) of the pairs at positions `kept`"""
        J, dl = solve(sums([self.pairs[a] for a in kept]), self.P)
        return J.v, 2 * J.e, [d.v for d in dl], [2 * d.e for d in dl]

    def eliminate(self):
        """the backward elimination in exact arithmetic: kept, order (positions in the order they left), rounds, decided"""
        kept = sorted(self.pairs); self.order = []; self.decided = self.sure; self.least = INF; self.loo = []
        while True:
            S = sums([self.pairs[a] for a in kept]); J, dl = solve(S, self.P); B = 2 * J.e
            g = mpf(self.gate[len(kept)])
            if kept:
                self.decided &= bool(abs(J.v - g) >= HEADROOM * B); self.least = min(self.least, float(abs(J.v - g) / B) if B > 0 else INF)
            if not kept or J.v < g:
                break
            cand = []
            for a in kept:
                Jr, _ = solve(without(S, self.pairs[a]), self.P); cand.append((Jr.v, a, 2 * Jr.e))
            cand.sort(key=lambda t: (t[0], t[1])); self.loo.append(cand)
            if len(cand) > 1:
                gap = cand[1][0] - cand[0][0]; Bb = cand[0][2] + cand[1][2]
                self.decided &= bool(gap >= HEADROOM * Bb); self.least = min(self.least, float(gap / Bb) if Bb > 0 else INF)
            self.order.append(cand[0][1]); kept = [a for a in kept if a != cand[0][1]]
        self.kept = kept; self.J, self.B = J.v, B; self.delta = [d.v for d in dl]; self.Bd = [2 * d.e for d in dl]
        self.rounds = len(self.order) + 1; self.eliminated = True
        return self

    def expect_index(self):
        return [self.hyp[a] if a in self.kept else -1 for a in range(self.k)]

    def failures(self, idx, J, n_kept, n_dropped, n_untestable, delta):
        """[what] of a device result (idx in the frame's order) the reference rejects; self.worst = |J - exact| / B of this result"""
        bad = []; idx = [int(j) for j in idx]; kept = []
        for a, j in enumerate(idx):
            if j == -1:
                continue
            if j != self.hyp[a]:
                bad.append("position %d: cone %d is not the hypothesis' %d" % (a, j, self.hyp[a]))
            elif a not in self.pairs:
                bad.append("position %d: an untestable pair is kept" % a) if self.sure else None
            else:
                kept.append(a)
        if bad:
            return bad
        if int(n_kept) != len(kept):
            bad.append("n_kept %d, the index keeps %d" % (n_kept, len(kept)))
        if int(n_kept) + int(n_dropped) + int(n_untestable) != self.n_named:
            bad.append("counts %d + %d + %d do not add up to %d" % (n_kept, n_dropped, n_untestable, self.n_named))
        if self.sure and int(n_untestable) != self.n_untestable:
            bad.append("n_untestable %d, the reference has %d" % (n_untestable, self.n_untestable))
        Jx, B, dx, Bd = self.J_of(kept)
        r = abs(mpf(float(J)) - Jx) / B if B > 0 else (mpf(0) if mpf(float(J)) == Jx else mpf(INF))
        self.worst = float(r)
        if not r <= 1:
            bad.append("J %.17g off the exact %.17g of the kept set by %.3g B" % (J, float(Jx), float(r)))
        for t in range(3):
            if not abs(mpf(float(delta[t])) - dx[t]) <= Bd[t]:
                bad.append("delta[%d] %.17g off the exact %.17g, B %.3g" % (t, delta[t], float(dx[t]), float(Bd[t])))
        if kept and not float(J) < self.gate[len(kept)]:
            bad.append("J %.17g is not below gate[%d] = %.17g" % (J, len(kept), self.gate[len(kept)]))
        if self.eliminated and self.decided:
            if idx != self.expect_index():
                bad.append("index %s, the reference keeps %s" % ([a for a in kept][:12], self.kept[:12]))
            if int(n_dropped) != len(self.order):
                bad.append("n_dropped %d, the reference dropped %d" % (n_dropped, len(self.order)))
        return bad


def brute(F, kept):
    """nu^T (blockdiag(D) + G Sigma_p G^T)^-1 nu over the stacked pairs at positions `kept`, dense, in mpmath"""
    n = len(kept)
    if n == 0:
        return mpf(0)
    S = MP.zeros(2 * n, 2 * n); nu = MP.zeros(2 * n, 1); G = MP.zeros(2 * n, 3)
    for t, a in enumerate(kept):
        pr = F.pairs[a]
        S[2 * t, 2 * t] = pr.D[0]; S[2 * t, 2 * t + 1] = S[2 * t + 1, 2 * t] = pr.D[1]; S[2 * t + 1, 2 * t + 1] = pr.D[2]
        nu[2 * t] = pr.nu[0]; nu[2 * t + 1] = pr.nu[1]
        G[2 * t, 0] = 1; G[2 * t + 1, 1] = 1; G[2 * t, 2] = pr.wp[0]; G[2 * t + 1, 2] = pr.wp[1]
    if F.P is not None:
        p00, p01, p02, p11, p12, p22 = F.P
        S = S + G * MP.matrix([[p00, p01, p02], [p01, p11, p12], [p02, p12, p22]]) * G.T
    return (nu.T * MP.lu_solve(S, nu))[0]


def make(case, hyp, frame_start, gate, order=None, R=None, cache=None):
    """the FrameRefs of a case dict (assoc_nn_shapes' layout: lidar, poses, pose_of, obs, map_xy, map_cov, pose_cov, params) whose observations,
    taken in `order` (None: as they are), form the frames of frame_start; hyp is in that order.  R: the case's frontend_exact_ref.Ref if the caller
    has it already; cache: a dict that keeps the pairs (observation, cone) from one call to the next"""
    R = fx.Ref(case["obs"], case["poses"], case["pose_of"], case["lidar"]) if R is None else R
    order = np.arange(len(case["obs"])) if order is None else np.asarray(order)
    p = nr.params_of(**case["params"]); out = []
    for f in range(len(frame_start) - 1):
        a, b = int(frame_start[f]), int(frame_start[f + 1]); mem = order[a:b]
        pi = int(case["pose_of"][mem[0]]) if b > a else 0
        assert all(int(case["pose_of"][i]) == pi for i in mem)
        pc = None if case["pose_cov"] is None else np.asarray(case["pose_cov"]).reshape(-1, 9)[pi]
        out.append(FrameRef(R, mem, hyp[a:b], case["poses"][pi] if len(case["poses"]) else np.zeros(3), pc, case["map_xy"], case["map_cov"], gate, p, cache))
    return out
