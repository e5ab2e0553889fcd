"""Frame localisation in exact arithmetic (TEST-ONLY; mpmath, 60 digits), written from include/graphslam.h ("frame localisation") — not from
the kernel — with the bounds the device is held to, and two checkers that do NOT repeat the iteration.

    x_0 = x0;  x_k = x0 + d_k;  pair terms at x_k (the joint test's, from the pose x_k without a pose covariance);  c, M, m_k summed;
    b = c (k = 0) or c + M d_k;  d_{k+1} = Sigma_p (I + M Sigma_p)^-1 b;  stop when every |d_{k+1} - d_k| is within its tolerance;
    final pass at x_f = x0 + d_f:  a, M;  cov = Sigma_p (I + M Sigma_p)^-1;  chi2 = a + x . d_f;  pose = (t0 + d_f, normalize_theta(theta0 + d_f2))

THE BOUND B.  u = 2^-53.  Every device quantity is carried as assoc_nn_ref.E = (exact value, e), |device - exact| <= 2 e to first order, by the
product, sum and quotient rules of assoc_nn_ref / joint_compat_ref.  The exact value is that of THIS iteration run in exact arithmetic from the
fp64 inputs.  What is new against joint_compat_ref: the pose of iteration k is itself an E (x0 + d_k, one addition, carrying e(d_k)), its
cos / sin are E(cos, |sin| e_theta + 4 u |cos|) and likewise (sincos counts 4 u as in assoc_nn_ref), and the query's side (w, g, Q) is formed
from those by assoc_nn_ref.Query's lines.  So e(d_k) enters iteration k through g (into nu, c) and through M d_k in b; the rules take absolute
values, so the two do not cancel as they do in exact arithmetic: e(d) may grow by a factor of about two per iteration — a pessimistic bound,
still first order, and with at most 16 iterations far below every tolerance used.  Sums: e(S) = sum e(t) + 10 u sum |t| (4 additions inside a
lane from +0, 6 butterfly levels).  The solve's operations one by one as in joint_compat_ref.solve, with b in place of c.  Final pass: the same
with a; cov_rs 5 operations and the division; chi2 6; the pose one addition, and 4 u |theta| more where normalize_theta acts.
B = 2 e per output.  Nothing here is fitted to a device output.

DECIDED.  A frame is DECIDED when every pair test of every pass is sure (valid query, det and D00 beyond their bands) and every stop
comparison — each |d_{k+1,r} - d_kr| against its tolerance, in every iteration — has 1000 B to spare (B = 2 e of that difference).  Only then
are `iterations` and `status` compared exactly.  run(force=n) makes exactly n solves whatever the stop tests say: the values and bounds a device
result with that iteration count is held to when the frame is not decided.

CHECKERS (no iteration).  step_at(pose): the exact Gauss-Newton step at a given pose, (Sigma_p^-1 + M)^-1 times the gradient, written d' - d with
d = pose - x0 and d' = Sigma_p (I + M Sigma_p)^-1 (c + M d) so that a singular Sigma_p is allowed; M and c are summed exactly from the pairs and the
3 x 3 system is solved densely (LU) in mpmath.  A frame reported converged must have |step| <= tolerance + B(pose) in each component.
cov_at(pose): the dense Sigma_p (I + M Sigma_p)^-1 at that pose; the reported covariance must lie within B(cov) of it.  step_at_mp and cov_meas_at
are the same two in MEASUREMENT space (the Kalman form, a 2n x 2n solve): an independent formula the CPU tests hold the others and the iteration to."""
import numpy as np

import assoc_nn_ref as nr
import frontend_exact_ref as fx
import joint_compat_ref as jr

MP, mpf, U, E, ediv = nr.MP, nr.mpf, nr.U, nr.E, jr.ediv
INF = float("inf")
HEADROOM = 1000
UP = ((0, 1, 2), (1, 3, 4), (2, 4, 5))                                       # the upper triangle's slot of entry (r, s)


def ecossin(th):
    cv, sv = MP.cos(th.v), MP.sin(th.v)
    return E(cv, abs(sv) * th.e + 4 * U * abs(cv)), E(sv, abs(cv) * th.e + 4 * U * abs(sv))


class Row:
    """what no iteration changes of one pair: z as E, the cone and its covariance as floats, the constants of Q; live False: it can never count"""

    def __init__(self, R, i, j, map_xy, map_cov, p):
        self.live = (not R.nan[i]) and 0 <= j < len(map_xy)
        if not self.live:
            return
        self.zx = E(mpf(R.z_hi[i, 0]) + mpf(R.z_lo[i, 0]), mpf(R.Bz[i, 0])); self.zy = E(mpf(R.z_hi[i, 1]) + mpf(R.z_lo[i, 1]), mpf(R.Bz[i, 1]))
        r2 = self.zx * self.zx + self.zy * self.zy
        if r2.v == 0:
            self.live = False
            return
        sr2 = E(p["sigma_range"]) * E(p["sigma_range"]); kv = sr2.v / r2.v
        self.k = E(kv, sr2.e / r2.v + kv * r2.e / r2.v + U * kv)
        self.sb2 = E(p["sigma_bearing"]) * E(p["sigma_bearing"]); self.sx2 = E(p["sigma_xy"]) * E(p["sigma_xy"])
        self.l = (float(map_xy[j][0]), float(map_xy[j][1])); self.cov = np.zeros(4) if map_cov is None else map_cov[j]
        if not (np.isfinite(self.l[0]) and np.isfinite(self.l[1])):           # nu is not finite: never counts
            self.live = False

    def terms(self, pose, c, s):
        """(counts, sure, the ten terms as E, (nu, D, wp) exact) at the pose (three E) whose heading has cos / sin (c, s)"""
        zx, zy, k, sb2, sx2 = self.zx, self.zy, self.k, self.sb2, self.sx2
        wx = zx * c - zy * s; wy = zx * s + zy * c
        gx = wx + pose[0]; gy = wy + pose[1]
        a00 = ((k * wx) * wx + (sb2 * wy) * wy) + sx2; a01 = (k * wx) * wy - (sb2 * wx) * wy; a11 = ((k * wy) * wy + (sb2 * wx) * wx) + sx2
        ux = (zx * s + zy * c).neg(); uy = zx * c - zy * s
        n0 = E(self.l[0]) - gx; n1 = E(self.l[1]) - gy
        d00 = E(self.cov[0]) + a00; d01 = E(self.cov[1]) + a01; d11 = E(self.cov[3]) + a11
        det = d00 * d11 - d01 * d01
        if not (det.v > 0 and d00.v > 0):
            return False, bool(det.v < -2 * det.e or d00.v < -2 * d00.e or (det.v == 0 and det.e == 0)), None, None
        if not (det.v > 4 * det.e and d00.v > 2 * d00.e):
            return False, False, None, None
        a = ediv(((d11 * n0) * n0 - (d01.twice() * n0) * n1) + (d00 * n1) * n1, det)
        y0 = ediv(d11 * n0 - d01 * n1, det); y1 = ediv(d00 * n1 - d01 * n0, det)
        e00 = ediv(d11, det); e01 = ediv(d01, det).neg(); e11 = ediv(d00, det)
        h0 = e00 * ux + e01 * uy; h1 = e01 * ux + e11 * uy
        return True, True, [a, y0, y1, ux * y0 + uy * y1, e00, e01, h0, e11, h1, ux * h0 + uy * h1], ((n0.v, n1.v), (d00.v, d01.v, d11.v), (ux.v, uy.v))


def sums(ts):
    out = []
    for q in range(10):
        v = mpf(0); e = mpf(0); ab = mpf(0)
        for t in ts:
            v += t[q].v; e += t[q].e; ab += abs(t[q].v)
        out.append(E(v, e + 10 * U * ab))
    return out


def cofactors(S, P):
    """(Sigma_p as a 3x3 of E, C, detA) from the sums' M and the upper triangle P — the header's operations"""
    m00, m01, m02, m11, m12, m22 = S[4:]
    M = [[m00, m01, m02], [m01, m11, m12], [m02, m12, m22]]; Pm = [[E(P[UP[r][s]]) for s in range(3)] for r in range(3)]
    A = [[(M[r][0] * Pm[0][s] + M[r][1] * Pm[1][s]) + M[r][2] * Pm[2][s] for s in range(3)] for r in range(3)]
    for r in range(3):
        A[r][r] = E(1) + A[r][r]
    C = [[None] * 3 for _ in range(3)]
    for r in range(3):
        for s in range(3):
            r1, r2 = (r + 1) % 3, (r + 2) % 3; s1, s2 = (s + 1) % 3, (s + 2) % 3
            C[r][s] = A[r1][s1] * A[r2][s2] - A[r1][s2] * A[r2][s1]
    det = (A[0][0] * C[0][0] + A[0][1] * C[0][1]) + A[0][2] * C[0][2]
    return M, Pm, C, det


def step(S, b, P):
    M, Pm, C, det = cofactors(S, P)
    x = [ediv((C[0][s] * b[0] + C[1][s] * b[1]) + C[2][s] * b[2], det) for s in range(3)]
    return x, [(Pm[r][0] * x[0] + Pm[r][1] * x[1]) + Pm[r][2] * x[2] for r in range(3)]


def normalize(th):
    """normalize_theta of an E; (E, sure): sure False when the branch cannot be told"""
    pi = MP.pi; e = th.e; sure = abs(abs(th.v) - pi) > 4 * (th.e + U * abs(th.v))
    if -pi <= th.v < pi:
        return th, sure
    v = th.v - MP.floor(th.v / (2 * pi)) * 2 * pi
    if v >= pi:
        v -= 2 * pi
    return E(v, e + 4 * U * abs(th.v)), sure


class Result:
    pass


class Frame:
    """one frame: members = observation numbers of R in the frame's order, hyp in that order, pose = x0 (three floats), pose_cov = 9 numbers or None"""

    def __init__(self, R, members, hyp, pose, pose_cov, map_xy, map_cov, p):
        self.x0 = [float(t) for t in pose]; self.P = jr.upper(pose_cov); self.k = len(members)
        map_xy = np.asarray(map_xy, dtype=np.float64).reshape(-1, 2); map_cov = None if map_cov is None else np.asarray(map_cov, dtype=np.float64).reshape(-1, 4)
        self.rows = [Row(R, int(i), int(j), map_xy, map_cov, p) for i, j in zip(members, hyp) if int(j) != -1]
        self.rows = [r for r in self.rows if r.live]

    def at(self, pose):
        """(sums, count, sure, [(nu, D, wp)]) at the pose (three E)"""
        c, s = ecossin(pose[2]); ts = []; sure = True; raw = []
        for r in self.rows:
            ok, su, t, x = r.terms(pose, c, s); sure &= su
            if ok:
                ts.append(t); raw.append(x)
        return sums(ts), len(ts), sure, raw

    def run(self, max_iterations=5, tol_xy=1e-6, tol_theta=1e-8, force=None):
        res = Result(); x0 = [E(t) for t in self.x0]; d = [E(0), E(0), E(0)]; x = None; iters = 0
        res.decided = True; res.least = INF; tols = (mpf(tol_xy), mpf(tol_xy), mpf(tol_theta))
        if self.k == 0:                                                       # an empty frame has no pose
            res.status, res.iterations, res.n_pairs = 2, 0, 0
            res.pose = [E(0)] * 3; res.cov = [E(0)] * 9; res.chi2 = E(0); res.d = d
            return res
        status = 0 if self.P is None else 1
        if self.P is not None:
            for k in range(max_iterations if force is None else force):
                pose = x0 if k == 0 else [x0[r] + d[r] for r in range(3)]
                S, cnt, sure, _ = self.at(pose); res.decided &= sure
                if k == 0 and cnt == 0:
                    status = 2
                    break
                M = [[S[4], S[5], S[6]], [S[5], S[7], S[8]], [S[6], S[8], S[9]]]
                b = S[1:4] if k == 0 else [S[1 + r] + ((M[r][0] * d[0] + M[r][1] * d[1]) + M[r][2] * d[2]) for r in range(3)]
                xn, dn = step(S, b, self.P); iters += 1; conv = True
                for r in range(3):
                    df = dn[r] - d[r]; margin = abs(abs(df.v) - tols[r]); B = 2 * df.e
                    res.decided &= bool(margin >= HEADROOM * B); res.least = min(res.least, float(margin / B) if B > 0 else INF)
                    conv &= bool(abs(df.v) <= tols[r])
                d, x = dn, xn
                if conv:
                    status = 0
                    if force is None:
                        break
                else:
                    status = 1
        res.status, res.iterations, res.d = status, iters, d
        if status == 2:
            res.n_pairs = 0; res.pose = x0; res.chi2 = E(0)
            res.cov = [E(self.P[UP[r][s]]) for r in range(3) for s in range(3)]
            return res
        xf = x0 if iters == 0 else [x0[r] + d[r] for r in range(3)]
        S, cnt, sure, _ = self.at(xf); res.decided &= sure; res.n_pairs = cnt
        th, sure = normalize(xf[2]); res.decided &= bool(sure)
        res.pose = [xf[0], xf[1], th]
        if self.P is None:
            res.cov = [E(0)] * 9; res.chi2 = S[0]
            return res
        _, Pm, C, det = cofactors(S, self.P)
        up = {}
        for r in range(3):
            for s in range(r, 3):
                up[(r, s)] = ediv((Pm[r][0] * C[s][0] + Pm[r][1] * C[s][1]) + Pm[r][2] * C[s][2], det)
        res.cov = [up[(min(r, s), max(r, s))] for r in range(3) for s in range(3)]
        res.chi2 = S[0] + ((x[0] * d[0] + x[1] * d[1]) + x[2] * d[2]) if iters > 0 else S[0]
        return res

    # ---- the checkers: dense, in measurement space, at a GIVEN pose (floats)
    def _dense(self, pose):
        pe = [E(t if isinstance(t, mpf) else mpf(float(t))) for t in pose]
        _, cnt, _, raw = self.at(pe)
        n = len(raw); S = MP.zeros(2 * n, 2 * n); nu = MP.zeros(2 * n, 1); G = MP.zeros(2 * n, 3)
        for t, (v, D, wp) in enumerate(raw):
            S[2 * t, 2 * t] = D[0]; S[2 * t, 2 * t + 1] = S[2 * t + 1, 2 * t] = D[1]; S[2 * t + 1, 2 * t + 1] = D[2]
            nu[2 * t] = v[0]; nu[2 * t + 1] = v[1]; G[2 * t, 0] = 1; G[2 * t + 1, 1] = 1; G[2 * t, 2] = wp[0]; G[2 * t + 1, 2] = wp[1]
        Pm = MP.matrix([[mpf(self.P[UP[r][s]]) for s in range(3)] for r in range(3)])
        return n, S + G * Pm * G.T, nu, G, Pm

    def diff(self, pose):
        """pose - x0, the heading's difference taken to (-pi, pi]"""
        d = [mpf(float(pose[r])) - mpf(self.x0[r]) for r in range(3)]
        while d[2] > MP.pi:
            d[2] -= 2 * MP.pi
        while d[2] <= -MP.pi:
            d[2] += 2 * MP.pi
        return d

    def _normal(self, pose):
        """(n, M, c, Sigma_p) at the pose: the 3 x 3 normal matrix and right-hand side summed exactly from the pairs' nu, D and wp"""
        pe = [E(t if isinstance(t, mpf) else mpf(float(t))) for t in pose]
        _, cnt, _, raw = self.at(pe); M = MP.zeros(3, 3); c = MP.zeros(3, 1)
        for v, D, wp in raw:
            Di = MP.inverse(MP.matrix([[D[0], D[1]], [D[1], D[2]]])); Gm = MP.matrix([[1, 0, wp[0]], [0, 1, wp[1]]])
            M += Gm.T * Di * Gm; c += Gm.T * Di * MP.matrix([v[0], v[1]])
        return len(raw), M, c, MP.matrix([[mpf(self.P[UP[r][s]]) for s in range(3)] for r in range(3)])

    def step_at(self, pose):
        """the exact Gauss-Newton step at the pose (floats; the heading's difference to x0 taken to (-pi, pi]): (Sigma_p^-1 + M)^-1 times the gradient,
        as Sigma_p (I + M Sigma_p)^-1 (c + M d) - d, solved densely: three mpf"""
        d = MP.matrix(self.diff(pose)); n, M, c, Pm = self._normal([mpf(self.x0[r]) + d[r] for r in range(3)])
        dn = Pm * MP.lu_solve(MP.eye(3) + M * Pm, c + M * d)
        return [dn[r] - d[r] for r in range(3)]

    def cov_at(self, pose):
        """the dense (Sigma_p^-1 + M)^-1 = Sigma_p (I + M Sigma_p)^-1 at the pose: nine mpf"""
        n, M, c, Pm = self._normal(pose); Cm = Pm * MP.inverse(MP.eye(3) + M * Pm)
        return [Cm[r, s] for r in range(3) for s in range(3)]

    def cov_meas_at(self, pose):
        """the same in measurement space, Sigma_p - Sigma_p G^T S^-1 G Sigma_p: nine mpf (small frames)"""
        n, S, nu, G, Pm = self._dense(pose)
        if n == 0:
            return [Pm[r, s] for r in range(3) for s in range(3)]
        Cm = Pm - Pm * G.T * MP.inverse(S) * G * Pm
        return [Cm[r, s] for r in range(3) for s in range(3)]

    def minimise(self, iterations=60):
        """the fixed point of the dense iteration from x0, to 40 digits: (pose as three mpf, steps taken)"""
        x = [mpf(t) for t in self.x0]
        for k in range(iterations):
            st = self.step_at_mp(x)
            x = [x[r] + st[r] for r in range(3)]
            if max(abs(t) for t in st) < mpf(10) ** -40:
                return x, k + 1
        raise AssertionError("the dense iteration did not settle")

    def step_at_mp(self, x):
        """the Gauss-Newton step at x (three mpf) in measurement space: Sigma_p G^T (blockdiag(D) + G Sigma_p G^T)^-1 (nu + G d) - d"""
        n, S, nu, G, Pm = self._dense(x); d = MP.matrix([x[r] - mpf(self.x0[r]) for r in range(3)])
        if n == 0:
            return [-d[r] for r in range(3)]
        dn = Pm * G.T * MP.lu_solve(S, nu + G * d)
        return [dn[r] - d[r] for r in range(3)]

    # ---- a device result against the reference
    def failures(self, rec, max_iterations=5, tol_xy=1e-6, tol_theta=1e-8, checkers=True):
        """[what] of a device record (pose [3], cov [9], chi2, n_pairs, iterations, status) the reference rejects; self.worst = the largest
        |device - exact| / B over its outputs, self.res = the exact run it was held to"""
        pose, cov, chi2, n_pairs, iters, status = rec; bad = []
        res = self.run(max_iterations, tol_xy, tol_theta); self.worst = 0.0
        if res.decided:
            if int(iters) != res.iterations or int(status) != res.status:
                bad.append("decided: iterations %d status %d, the reference has %d and %d" % (iters, status, res.iterations, res.status))
        elif int(status) in (0, 1) and 1 <= int(iters) <= max_iterations and int(iters) != res.iterations:
            res = self.run(max_iterations, tol_xy, tol_theta, force=int(iters))
        self.res = res
        if bad or int(status) != res.status and res.decided:
            return bad
        if int(status) not in (0, 1, 2):
            return ["status %d" % status]
        if int(n_pairs) != res.n_pairs and res.decided:
            bad.append("n_pairs %d, the reference counts %d" % (n_pairs, res.n_pairs))

        def hold(name, got, ex):
            B = 2 * ex.e; dv = abs(mpf(float(got)) - ex.v)
            r = float(dv / B) if B > 0 else (0.0 if dv == 0 else INF)
            self.worst = max(self.worst, r)
            if not r <= 1:
                bad.append("%s %.17g off the exact %.17g by %.3g B (B %.3g)" % (name, got, float(ex.v), r, float(B)))
        for r in range(3):
            hold("pose[%d]" % r, pose[r], res.pose[r])
        for r in range(9):
            hold("cov[%d]" % r, cov[r], res.cov[r])
        hold("chi2", chi2, res.chi2)
        if checkers and self.P is not None and int(status) == 0 and res.status == 0 and int(iters) > 0:
            st = self.step_at(pose); tols = (tol_xy, tol_xy, tol_theta)
            for r in range(3):
                if not abs(st[r]) <= mpf(tols[r]) + 2 * res.pose[r].e:
                    bad.append("the exact step at the returned pose: component %d is %.3g, tolerance %.3g + B %.3g" % (r, float(st[r]), tols[r], float(2 * res.pose[r].e)))
        if checkers and self.P is not None and int(status) in (0, 1) and int(iters) > 0:
            cv = self.cov_at(pose)
            for r in range(9):
                if not abs(mpf(float(cov[r])) - cv[r]) <= 2 * res.cov[r].e:
                    bad.append("cov[%d] %.17g off the dense %.17g, B %.3g" % (r, cov[r], float(cv[r]), float(2 * res.cov[r].e)))
        return bad


def make(case, hyp, frame_start, order=None, R=None):
    """the Frames of a case dict (assoc_nn_shapes' layout) whose observations, taken in `order`, form the frames of frame_start; hyp in that order"""
    R = fx.Ref(case["obs"], case["poses"], case["pose_of"], case["lidar"]) if R is None else R
    order = np.arange(len(case["obs"])) if order is None else np.asarray(order)
    p = nr.params_of(**case["params"]); out = []
    for f in range(len(frame_start) - 1):
        a, b = int(frame_start[f]), int(frame_start[f + 1]); mem = order[a:b]
        pi = int(case["pose_of"][mem[0]]) if b > a else 0
        pc = None if case["pose_cov"] is None else np.asarray(case["pose_cov"]).reshape(-1, 9)[pi]
        out.append(Frame(R, mem, hyp[a:b], case["poses"][pi] if len(case["poses"]) else np.zeros(3), pc, case["map_xy"], case["map_cov"], p))
    return out
