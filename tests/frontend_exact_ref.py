"""The exact front end (TEST-ONLY; mpmath, 60 digits) and the bounds its device paths are held to: A0 (k_polar_to_xy, k_cone_to_global, the
conversions inside k_associate, k_associate_grid_dev and k_frame_frontend) entry by entry, A1 as a set of admissible indices per query.

Written from include/graphslam.h (front-end section) and the kernel comments — not from the kernels' code, not from the oracle:
    A0   sign = az / |az| (NaN at az == 0),  ang = kPiF - |az kDeg2Rad|,  dnew = sqrt(lidar^2 + dist^2 - 2 lidar dist cos(ang)),
         t = sin(ang) dist / dnew,  az2 = asin(t) kRad2Deg sign,  (x, y) = dnew cos(zen kDeg2Rad) (cos, sin)(az2 kDeg2Rad)
         global: (gx, gy) = R(theta) (x, y) + (px, py)
    A1   the LOWEST map index j with |type_j - type_i| < type_tol (localizer: (type_j - (int)type_i) < type_tol) and
         sqrt(dx^2 + dy^2) < threshold, else -1
kPiF is the FLOAT 3.14159265f widened, kDeg2Rad = 0.017453292522222 and kRad2Deg = 57.295779513082325 are the doubles the kernels use; every
input is the fp64 number the handle is given, taken exactly.  In exact arithmetic dnew^2 - (sin(ang) dist)^2 = (lidar - dist cos(ang))^2, so
|t| <= 1 with equality where the cone is abeam of the CoG (dist cos(az) = -lidar): the asin's branch point.

The bound of A0, |got - exact| <= B per entry, u = 2^-53.  The count of roundings in units of u, one line per step, magnitudes to first
order; device sincos / cos 4, asin 4 (the OpenCL fp64 table side_exact_ref uses), sqrt and division correctly rounded; the total doubled
(second order, and an ulp of a result is 2 u of it), as C(n) = 2 (L + n) in the other references:
    a1    = |az kDeg2Rad|          product 1                                                    d_a1   = a1
    ang   = kPiF - a1              a1, subtraction 1                                            d_ang  = a1 + |ang|
    sa,ca = sincos(ang)            the argument through the derivative, sincos 4                d_sa   = |ca| d_ang + 4 |sa|   (d_ca likewise)
    q     = l^2 + d^2 - 2 l d ca   squares 1, addition 1, subtraction 1 = 3 on l^2 + d^2;       d_q    = 3 (l^2 + d^2 + 2 l d |ca|) + 2 l d d_ca
                                   2 l d: 1 (2 l is exact), times ca 1, subtraction 1 = 3
    dnew  = sqrt(q)                q through 1 / (2 dnew), sqrt 1                               d_dnew = d_q / (2 dnew) + dnew
    t     = sa d / dnew            product 1, division 1                                        d_t    = (d d_sa + |sa d|) / dnew + |t| d_dnew / dnew + |t|
    THE ASIN STEP is not linearised: with Dt = 2 u d_t the rest of the formula is evaluated at t, t - Dt and t + Dt, clipped to [-1, 1] (cos and
    sin of kRad2Deg kDeg2Rad asin(t) are monotone in t on either side of 0, so the ends give the largest deviation), and the bound is the
    larger deviation plus the first-order rest at that point:
    phi   = asin(t) kRad2Deg sign kDeg2Rad      asin 4, two products 2 (sign is exactly +-1)    d_phi  = 6 |phi|
    c2,s2 = sincos(phi)                                                                         d_c2   = |s2| d_phi + 4 |c2|   (d_s2 likewise)
    cz    = cos(zen kDeg2Rad)      product 1 through the derivative, cos 4                      d_cz   = |sin(zr)| |zr| + 4 |cz|
    x     = dnew cz c2             two products 2                                               d_x    = |cz c2| d_dnew + |dnew c2| d_cz + |dnew cz| d_c2 + 2 |x|
    B_x   = max over the three points of |x(t') - x(t)| + 2 u d_x(t')                           (y with s2 for c2)
An entry with |t| + Dt >= 1 is in the BRANCH BAND: the device's t may exceed 1 in its last places, and asin gives NaN.  There the device may
return NaN in both x and y, or numbers inside B (which, through the clipping, reaches the branch point); anything else fails.  Outside the band
a NaN fails.  az == 0 (either sign) and lidar == dist == 0 are NaN in the formula itself: NaN in both is then the only admissible answer.
Refusal (an assertion, as the other references do at a branch point): 2 u d_dnew / dnew >= 1e-3, where "first order" ends for 1 / dnew.

The global XY:  gx = (x c - y s) + px with c, s of the pose: cos / sin 4, product 1, subtraction 1, addition 1
    B_gx  = 2 u (7 (|x c| + |y s|) + |px|) + |c| B_x + |s| B_y                                   (gy likewise; a NaN of x, y is a NaN of both)

A1.  The device's distance to a cone differs from the exact one by at most
    band  = B_gx + B_gy + 8 u thr        (d is 1-Lipschitz in (dx, dy); dx 1, square 1, sum 1, sqrt 1 = 3 u d, doubled, for d <= 4/3 thr)
and its answer is one of: the lowest index m* whose exact distance is below thr - band and whose type test (exact in fp64 for the integer
types used) passes; an index below m* with a passing type test and an exact distance within +-band of thr; -1 where no m* exists (then any
in-band index as well).  A query whose exact XY is NaN gives -1.  A query in the A0 branch band carries its wider B into band, and -1 is
admissible for it exactly when the path's own reported global XY is NaN (check_index's `reported_nan`).  thr <= 0 or NaN: -1 everywhere.
Distances are screened in fp64 (error below 16 u (|m| + |g|), far inside the 8 band + 32 u (|m| + |g|) margin used) and only pairs within the
margin of thr are taken to mpmath."""
import numpy as np

import lin_exact_ref as lx

MP, mpf, U = lx.MP, lx.mpf, lx.U
K_PIF = mpf(float(np.float32(3.14159265)))
K_D2R = mpf(0.017453292522222)
K_R2D = mpf(57.295779513082325)
ONE = mpf(1)
NAN = float("nan")


def _split(v):
    hi = float(v)
    return hi, float(v - mpf(hi))


def a0_entry(az, zen, dist, lidar):
    """one observation: dict(x, y: mpf or None (NaN), Bx, By: mpf, band: bool, t)"""
    az, zen, dist, l = mpf(float(az)), mpf(float(zen)), mpf(float(dist)), mpf(float(lidar))
    if az == 0 or (dist == 0 and l == 0) or not (MP.isfinite(az) and MP.isfinite(zen) and MP.isfinite(dist)):
        return dict(x=None, y=None, Bx=mpf(0), By=mpf(0), band=False, t=None)
    sign = 1 if az > 0 else -1
    a1 = abs(az * K_D2R); ang = K_PIF - a1
    sa, ca = MP.sin(ang), MP.cos(ang)
    d_ang = a1 + abs(ang)
    d_sa = abs(ca) * d_ang + 4 * abs(sa); d_ca = abs(sa) * d_ang + 4 * abs(ca)
    ld2 = 2 * l * dist
    q = l * l + dist * dist - ld2 * ca
    assert q > 0, ("dnew is exactly zero", float(az), float(dist))
    d_q = 3 * (l * l + dist * dist + ld2 * abs(ca)) + ld2 * d_ca
    dnew = MP.sqrt(q)
    d_dnew = d_q / (2 * dnew) + dnew
    assert 2 * U * d_dnew / dnew < 1e-3, ("the error of dnew is not small against dnew", float(az), float(dist), float(dnew))
    num = sa * dist
    t = num / dnew
    d_t = (dist * d_sa + abs(num)) / dnew + abs(t) * d_dnew / dnew + abs(t)
    Dt = 2 * U * d_t
    zr = zen * K_D2R; cz = MP.cos(zr); d_cz = abs(MP.sin(zr)) * abs(zr) + 4 * abs(cz)
    k = K_R2D * K_D2R * sign

    def at(tp):
        phi = MP.asin(tp) * k
        c2, s2 = MP.cos(phi), MP.sin(phi)
        d_phi = 6 * abs(phi)
        d_c2 = abs(s2) * d_phi + 4 * abs(c2); d_s2 = abs(c2) * d_phi + 4 * abs(s2)
        x, y = dnew * cz * c2, dnew * cz * s2
        d_x = abs(cz * c2) * d_dnew + abs(dnew * c2) * d_cz + abs(dnew * cz) * d_c2 + 2 * abs(x)
        d_y = abs(cz * s2) * d_dnew + abs(dnew * s2) * d_cz + abs(dnew * cz) * d_s2 + 2 * abs(y)
        return x, y, 2 * U * d_x, 2 * U * d_y

    x, y, ex, ey = at(t)
    Bx, By = ex, ey
    for tp in (max(t - Dt, -ONE), min(t + Dt, ONE)):
        xp, yp, exp_, eyp = at(tp)
        Bx = max(Bx, abs(xp - x) + exp_); By = max(By, abs(yp - y) + eyp)
    return dict(x=x, y=y, Bx=Bx, By=By, band=bool(abs(t) + Dt >= 1), t=t)


class Ref:
    """the exact A0 of a case: z (CoG frame) and g (global) as fp64 pairs hi + lo, their bounds, the NaN and branch-band flags"""

    def __init__(self, obs, poses, pose_of, lidar):
        obs = np.asarray(obs, dtype=np.float64).reshape(-1, 4); poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
        n = len(obs)
        self.n = n; self.obs = obs; self.poses = poses; self.pose_of = np.asarray(pose_of, dtype=np.int64); self.lidar = float(lidar)
        self.z_hi = np.full((n, 2), NAN); self.z_lo = np.zeros((n, 2)); self.Bz = np.zeros((n, 2))
        self.g_hi = np.full((n, 2), NAN); self.g_lo = np.zeros((n, 2)); self.Bg = np.zeros((n, 2))
        self.nan = np.zeros(n, dtype=bool); self.band = np.zeros(n, dtype=bool); self.t = np.full(n, NAN)
        trig = [(MP.cos(mpf(float(p[2]))), MP.sin(mpf(float(p[2])))) for p in poses]
        up = 1.0 + 1e-12                                                  # the bounds are rounded to fp64: upwards
        for i in range(n):
            e = a0_entry(obs[i, 0], obs[i, 1], obs[i, 2], lidar)
            if e["x"] is None:
                self.nan[i] = True
                continue
            x, y, Bx, By = e["x"], e["y"], e["Bx"], e["By"]
            self.band[i] = e["band"]; self.t[i] = float(e["t"])
            self.z_hi[i, 0], self.z_lo[i, 0] = _split(x); self.z_hi[i, 1], self.z_lo[i, 1] = _split(y)
            self.Bz[i] = float(Bx) * up, float(By) * up
            p = poses[self.pose_of[i]]; c, s = trig[self.pose_of[i]]; px, py = mpf(float(p[0])), mpf(float(p[1]))
            gx, gy = x * c - y * s + px, x * s + y * c + py
            Bgx = 2 * U * (7 * (abs(x * c) + abs(y * s)) + abs(px)) + abs(c) * Bx + abs(s) * By
            Bgy = 2 * U * (7 * (abs(x * s) + abs(y * c)) + abs(py)) + abs(s) * Bx + abs(c) * By
            self.g_hi[i, 0], self.g_lo[i, 0] = _split(gx); self.g_hi[i, 1], self.g_lo[i, 1] = _split(gy)
            self.Bg[i] = float(Bgx) * up, float(Bgy) * up
        self._adm = {}

    def band_of(self, thr):
        """the association band per query (module docstring)"""
        return (self.Bg[:, 0] + self.Bg[:, 1]) + 8 * U * abs(float(thr))

    def admissible(self, map_xy, map_type, thr, tol, signed=False, key=None):
        k = (key, float(thr), float(tol), bool(signed))
        if key is None or k not in self._adm:
            a = Admissible(self, map_xy, map_type, thr, tol, signed)
            if key is None:
                return a
            self._adm[k] = a
        return self._adm[k]


def _err(got, hi, lo):
    """|got - (hi + lo)| in fp64: got - hi is exact where it matters (Sterbenz), so the error of this is a few u of the result"""
    return np.abs((got - hi) - lo)


def check_xy(got, hi, lo, B, nan, band, tag=""):
    """an [n, 2] device array against the exact one.  Returns dict(worst: largest err / B outside the branch band, worst_band: the same over
    band entries that came back as numbers, band_nan / band_num: how the band entries came back); asserts the rules of the module docstring"""
    got = np.asarray(got, dtype=np.float64).reshape(-1, 2)
    assert got.shape == hi.shape, (tag, got.shape, hi.shape)
    gn = np.isnan(got)
    bad = np.flatnonzero(nan & ~gn.all(axis=1))
    assert not len(bad), (tag, "the formula gives NaN here, the device a number", int(bad[0]), got[bad[0]].tolist())
    bad = np.flatnonzero(gn.any(axis=1) & ~gn.all(axis=1))
    assert not len(bad), (tag, "NaN in one of x, y only", int(bad[0]), got[bad[0]].tolist())
    bad = np.flatnonzero(gn.all(axis=1) & ~nan & ~band)
    assert not len(bad), (tag, "NaN outside the branch band", int(bad[0]))
    num = ~gn.all(axis=1) & ~nan
    with np.errstate(divide="ignore", invalid="ignore"):
        e = _err(got, hi, lo)
        r = np.where(B > 0, e / B, np.where(e == 0, 0.0, np.inf))
    r = np.where(num[:, None], r, 0.0)
    bad = np.argwhere(r > 1.0)
    assert not len(bad), (tag, "entry", bad[0].tolist(), "got", float(got[tuple(bad[0])]), "exact", float(hi[tuple(bad[0])]),
                          "err / B", float(r[tuple(bad[0])]), "in band", bool(band[bad[0][0]]))
    out = dict(worst=float(r[num & ~band].max()) if (num & ~band).any() else 0.0,
               worst_band=float(r[num & band].max()) if (num & band).any() else 0.0,
               band_nan=int((band & gn.all(axis=1)).sum()), band_num=int((band & num).sum()))
    return out


class Admissible:
    """per query the admissible answers of A1 on one map: mstar (-1: none), extra (query -> in-band indices below mstar), and the census of
    in-band candidates (n_inband: pairs with a passing type test within +-band of thr, below mstar)"""

    def __init__(self, R, map_xy, map_type, thr, tol, signed=False):
        map_xy = np.asarray(map_xy, dtype=np.float64).reshape(-1, 2); map_type = np.asarray(map_type, dtype=np.int64).reshape(-1)
        n, m = R.n, len(map_xy); thr = float(thr); tol = float(tol)
        self.n = n; self.R = R; self.thr = thr
        self.mstar = np.full(n, -1, dtype=np.int64); self.extra = {}; self.n_inband = 0; self.n_exact_pairs = 0
        self.band = R.band_of(thr)
        if m == 0 or not thr > 0:
            return
        ty = R.obs[:, 3]
        if signed:
            ok = (map_type[None, :] - ty.astype(np.int64)[:, None]).astype(np.float64) < tol
        else:
            ok = np.abs(map_type[None, :].astype(np.float64) - ty[:, None]) < tol
        ok &= ~R.nan[:, None]
        with np.errstate(invalid="ignore", over="ignore"):
            dx = map_xy[None, :, 0] - R.g_hi[:, None, 0]; dy = map_xy[None, :, 1] - R.g_hi[:, None, 1]
            D = np.sqrt(dx * dx + dy * dy)
            scale = np.abs(map_xy).max(axis=1)[None, :] + np.abs(R.g_hi).max(axis=1)[:, None]
            margin = 8 * self.band[:, None] + 32 * U * np.where(np.isfinite(scale), scale, 0.0)
            strict = ok & (D < thr - margin)
            near = ok & (np.abs(D - thr) <= margin)
        inband = np.zeros_like(ok)
        T = mpf(thr)
        for i, j in np.argwhere(near):
            gx = mpf(R.g_hi[i, 0]) + mpf(R.g_lo[i, 0]); gy = mpf(R.g_hi[i, 1]) + mpf(R.g_lo[i, 1])
            d = MP.sqrt((mpf(map_xy[j, 0]) - gx) ** 2 + (mpf(map_xy[j, 1]) - gy) ** 2)
            b = mpf(self.band[i]); self.n_exact_pairs += 1
            if d < T - b:
                strict[i, j] = True
            elif d <= T + b:
                inband[i, j] = True
        has = strict.any(axis=1)
        self.mstar = np.where(has, strict.argmax(axis=1), -1)
        for i in np.flatnonzero(inband.any(axis=1)):
            js = np.flatnonzero(inband[i]); js = js[js < self.mstar[i]] if has[i] else js
            if len(js):
                self.extra[int(i)] = set(int(j) for j in js); self.n_inband += len(js)

    def failures(self, got, reported_nan=None):
        """the queries whose device answer is not admissible (reported_nan: per query, whether the path's own global XY is NaN)"""
        got = np.asarray(got, dtype=np.int64).reshape(-1)
        assert len(got) == self.n, (len(got), self.n)
        R = self.R
        bad = []
        for i in np.flatnonzero(got != self.mstar):
            i = int(i)
            if got[i] in self.extra.get(i, ()):
                continue
            if got[i] == -1 and i in self.extra and self.mstar[i] == -1:
                continue
            if got[i] == -1 and R.band[i] and reported_nan is not None and reported_nan[i]:
                continue
            bad.append(i)
        if reported_nan is not None:                                       # a NaN query matches nothing, on any path
            bad += [int(i) for i in np.flatnonzero(np.asarray(reported_nan) & (got != -1))]
        return sorted(set(bad))

    def check(self, got, reported_nan=None, tag=""):
        bad = self.failures(got, reported_nan)
        if bad:
            i = bad[0]
            raise AssertionError((tag, "query", i, "got", int(np.asarray(got).reshape(-1)[i]), "lowest admissible", int(self.mstar[i]),
                                  "in band", sorted(self.extra.get(i, ())), "A0 band", bool(self.R.band[i]), "%d queries fail" % len(bad)))
        return True
