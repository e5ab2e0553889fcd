"""Test-only references that do not depend on the conditioning of the system (TEST-ONLY; nothing in the package imports it).

The parity tests compare one fp64 solve with another, so their tolerances are set by cond(H).  These helpers measure the arithmetic of
a solve instead, from the system the device itself factorised:

  - error-free transformations (TwoSum; TwoProd by Veltkamp splitting) and, on them, row sums that are accurate to about one rounding
    whatever the cancellation (SumK of Ogita, Rump and Oishi, vectorised over the rows of a sparse matrix);
  - the residual r = H x - b of the block-sparse normal equations that gs_export_system returns (the sign of
    test_gpu_parity.normal_equation_residual), duplicate edges summed exactly, fixed vertices (gidx < 0) dropped as the plan drops them;
  - the componentwise (Oettli-Prager) backward error  omega(x) = max_i |r_i| / (|H| |x| + |b|)_i  (0 / 0 counts as 0);
  - columns of H^-1 by iterative refinement: a double inverse as the approximate solver, residuals I - H X in double-double;
  - the first-order componentwise bound of Sigma = H^-1:  B = |Sigma| |H| |Sigma|.  Since Sigma H Sigma = Sigma, B_ij >= |Sigma_ij|: a bound
    C u B_ij never asks for better than C u relative, and is wider only where the entry is itself ill-conditioned.
"""
import numpy as np

U = 2.0 ** -53                                          # unit roundoff of binary64
_SPLIT = 134217729.0                                    # 2^27 + 1 (Veltkamp)


def two_sum(a, b):
    """s + e == a + b exactly, s = fl(a + b) (Knuth)"""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = _SPLIT * a
    hi = c - (c - a)
    return hi, a - hi


def two_prod(a, b):
    """p + e == a * b exactly, p = fl(a * b) (Dekker; no FMA needed)"""
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


class RowSums:
    """Sums of terms grouped by row, each to about one rounding of the exact sum (SumK, K = 3 by default).

    rows: the row of every term.  The terms of a row are laid out contiguously (stable in their given order); VecSum runs over every
    row at once, one position of the rows at a time — the rows sorted by length so that the active ones are a prefix."""

    def __init__(self, rows, n):
        rows = np.asarray(rows, dtype=np.int64)
        self.n = n
        self.order = np.argsort(rows, kind="stable")
        self.cnt = np.bincount(rows, minlength=n)
        self.start = np.concatenate([[0], np.cumsum(self.cnt)[:-1]]).astype(np.int64)
        by = np.argsort(-self.cnt, kind="stable")
        self._cs, self._st = self.cnt[by], self.start[by]
        self._live = self.cnt > 0

    def _vecsum(self, T):
        cs, st = self._cs, self._st
        for t in range(1, int(cs[0]) if len(cs) else 0):
            m = int(np.searchsorted(-cs, -t, side="left"))          # rows with more than t terms
            i = st[:m] + t
            s, e = two_sum(T[i], T[i - 1])
            T[i] = s; T[i - 1] = e

    def __call__(self, terms, K=3):
        """terms: [n_terms] or [n_terms, k] in the order of `rows`; returns [n] or [n, k]"""
        T = np.array(terms, dtype=np.float64)[self.order]
        for _ in range(K - 1):
            self._vecsum(T)
        out = np.zeros((self.n,) + T.shape[1:])
        if not self._live.any():
            return out
        st, cnt = self.start[self._live], self.cnt[self._live]
        last = st + cnt - 1
        s = T[last].copy(); T[last] = 0.0
        out[self._live] = s + np.add.reduceat(T, st, axis=0)       # the error terms in plain double, then the sum itself
        return out


class Sparse:
    """A square matrix as a list of (row, col, value) terms, duplicates kept (they are summed exactly by RowSums)"""

    def __init__(self, rows, cols, vals, n):
        self.rows = np.asarray(rows, dtype=np.int64); self.cols = np.asarray(cols, dtype=np.int64)
        self.vals = np.asarray(vals, dtype=np.float64); self.n = int(n)
        self._sums = None

    def sums(self):
        """row sums over [products (p), their errors (e), one constant per row]"""
        if self._sums is None:
            ar = np.arange(self.n)
            self._sums = RowSums(np.concatenate([self.rows, self.rows, ar]), self.n)
        return self._sums

    def dense(self):
        A = np.zeros((self.n, self.n))
        np.add.at(A, (self.rows, self.cols), self.vals)
        return A

    def abs_dense(self):
        A = np.zeros((self.n, self.n))
        np.add.at(A, (self.rows, self.cols), np.abs(self.vals))
        return A

    def residual(self, X, C, K=3):
        """H X - C, X and C [n] or [n, k]: every product split exactly, each row summed by SumK"""
        p, e = two_prod(self.vals.reshape((-1,) + (1,) * (X.ndim - 1)), X[self.cols])
        return self.sums()(np.concatenate([p, e, -np.asarray(C, dtype=np.float64)]), K=K)

    def abs_product(self, X, C, K=2):
        """|H| |X| + |C| (no cancellation: SumK with K = 2 is a few ulps already)"""
        p, e = two_prod(np.abs(self.vals).reshape((-1,) + (1,) * (X.ndim - 1)), np.abs(X[self.cols]))
        return self.sums()(np.concatenate([p, e, np.abs(np.asarray(C, dtype=np.float64))]), K=K)


def backward_error(H, x, b):
    """omega(x) = max_i |H x - b|_i / (|H| |x| + |b|)_i; a row whose numerator and denominator are both 0 counts as 0"""
    x = np.asarray(x, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    r = np.abs(H.residual(x, b)); d = H.abs_product(x, b)
    if not len(r):
        return 0.0
    q = np.where(d > 0, r / np.where(d > 0, d, 1.0), np.where(r > 0, np.inf, 0.0))
    return float(q.max())


class BlockSystem:
    """The scalar system of an export_system() dict (array-of-blocks, insertion order) over the free vertices, numbered like the plan:
    a pose's scalars start at pose_gidx[p], a landmark's at lm_gidx[l]; gidx < 0: fixed, its rows and columns dropped."""

    def __init__(self, sysm, g, pose_gidx, lm_gidx):
        pg = np.asarray(pose_gidx, dtype=np.int64); lg = np.asarray(lm_gidx, dtype=np.int64)
        self.pose_gidx, self.lm_gidx = pg, lg
        self.n = max(int(pg.max()) + 3 if (pg >= 0).any() else 0, int(lg.max()) + 2 if (lg >= 0).any() else 0)
        R, Cc, V = [], [], []

        def add(gr, wr, gc, wc, blocks):                # blocks [E, wr, wc] at rows gr (width wr), columns gc
            ok = (gr >= 0) & (gc >= 0)
            gr, gc, blocks = gr[ok], gc[ok], blocks[ok]
            for a in range(wr):
                for c in range(wc):
                    R.append(gr + a); Cc.append(gc + c); V.append(blocks[:, a, c])
        add(pg, 3, pg, 3, sysm["Hpp_diag"].reshape(-1, 3, 3))
        add(lg, 2, lg, 2, sysm["Hll_diag"].reshape(-1, 2, 2))
        pi, pj = np.asarray(g["pp_i"], dtype=np.int64), np.asarray(g["pp_j"], dtype=np.int64)
        Ho = sysm["Hpp_off"].reshape(-1, 3, 3)             # rows = pose i, columns = pose j
        add(pg[pi], 3, pg[pj], 3, Ho); add(pg[pj], 3, pg[pi], 3, Ho.transpose(0, 2, 1))
        pp, pl = np.asarray(g["pl_p"], dtype=np.int64), np.asarray(g["pl_l"], dtype=np.int64)
        Hl = sysm["Hpl"].reshape(-1, 3, 2)                 # rows = pose, columns = landmark
        add(pg[pp], 3, lg[pl], 2, Hl); add(lg[pl], 2, pg[pp], 3, Hl.transpose(0, 2, 1))
        cat = lambda a: np.concatenate(a) if a else np.zeros(0)
        self.H = Sparse(cat(R).astype(np.int64), cat(Cc).astype(np.int64), cat(V), self.n)
        self.b = self.scatter(sysm["b_pose"], sysm["b_lm"])

    def scatter(self, vp, vl):
        """per-vertex arrays [N, 3], [M, 2] -> the scalar vector of the free vertices"""
        out = np.zeros(self.n)
        for gidx, v, w in ((self.pose_gidx, vp, 3), (self.lm_gidx, vl, 2)):
            v = np.asarray(v, dtype=np.float64).reshape(-1, w); ok = gidx >= 0
            for c in range(w):
                out[gidx[ok] + c] = v[ok, c]
        return out

    def residual(self, dp, dl):
        return self.H.residual(self.scatter(dp, dl), self.b)

    def omega(self, dp, dl):
        return backward_error(self.H, self.scatter(dp, dl), self.b)


def refine_columns(H, cols, X0, steps=3, chunk=64):
    """Columns `cols` of H^-1, refined: X = X0[:, cols], then `steps` times X += X0 (E - H X) with the residual in double-double.
    X0: an approximate inverse in double (np.linalg.inv).  Each step contracts the error by about cond(H) u."""
    cols = np.asarray(cols, dtype=np.int64)
    out = np.zeros((H.n, len(cols)))
    for a in range(0, len(cols), chunk):
        cc = cols[a:a + chunk]
        E = np.zeros((H.n, len(cc))); E[cc, np.arange(len(cc))] = 1.0
        X = X0[:, cc].copy()
        for _ in range(steps):
            X = X - X0 @ H.residual(X, E, K=2)
        out[:, a:a + chunk] = X
    return out


def refined_inverse(H, steps=3):
    """H^-1 of a system of at most ~1 500 scalars, every column refined (refine_columns)"""
    X0 = np.linalg.inv(H.dense())
    X0 = (X0 + X0.T) / 2
    return refine_columns(H, np.arange(H.n), X0, steps=steps), X0


def sigma_bound(H, X0, cols):
    """B[:, cols] = |Sigma| |H| |Sigma[:, cols]| (from the unrefined inverse: B only scales the bound)"""
    A = np.abs(X0)
    return A @ (H.abs_dense() @ A[:, cols])
