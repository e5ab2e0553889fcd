"""numpy replay of the selected inversion (TEST-ONLY checker of gs_compute_marginals' index maps).

On top of plan_exec.Plan: factorise H front by front as the plan says, then run the Takahashi recursion from the root
to the leaves as the device kernels do (k_selinv_panel: the same recursion blocked in panels) — the boundary block of a front gathered from its parent's image through
the child map, then the pivots from the last to the first — and read covariance blocks out of the front images the way
the host's extraction tables do (the front that has the lower scalar as a pivot, the higher one among its rows).
It is not product code and nothing in the package imports it.
"""
import numpy as np

from oracle.pyoracle import _i
from plan_exec import Plan  # noqa: F401  (the plan object these functions take)


def factor(P, blocks):
    """Cholesky factor per front (plan_exec's replay of the iteration's factor): list of (f+1) x npiv panels, ok"""
    Hpl, Hpp_off = P._device_blocks(blocks)
    S = P.n_fronts
    Ls, Us, ok = [None] * S, [None] * S, True
    for s in range(S):
        F = P._assemble(s, blocks, Hpl, Hpp_off)
        P._extend_add(s, F, Us, lambda c: True)
        Ls[s], Us[s], good = P._factor(s, F)
        ok = ok and good
    return Ls, ok


def selinv(P, Ls):
    """Sigma image (dense, symmetric f x f) of every front, from the Cholesky panels: l = L[:, k] / L_kk, d = L_kk^2 — the unit-diagonal
    factor of the same H, i.e. what the device's LDL^T form (pivots captured) and its L L^T form (scaled on load) both feed the recursion"""
    S = P.n_fronts
    Sig = [None] * S
    for s in range(S - 1, -1, -1):
        npv, nb = int(P.npiv[s]), int(P.nbnd[s])
        f = npv + nb
        L = Ls[s][:f, :npv]
        X = np.zeros((f, f))
        if nb:
            m = P.child_map[P.map_off[s]:P.map_off[s] + nb]
            X[npv:, npv:] = Sig[int(P.parent[s])][np.ix_(m, m)]
        for k in range(npv - 1, -1, -1):
            lk = L[k + 1:, k] / L[k, k]; dinv = 1.0 / (L[k, k] * L[k, k])
            col = -X[k + 1:, k + 1:] @ lk
            X[k + 1:, k] = col; X[k, k + 1:] = col
            X[k, k] = dinv - lk @ col
        Sig[s] = X
    return Sig


class Rows:
    """scalar -> (front that has it as a pivot); (front, scalar) -> row of the front"""
    def __init__(self, P):
        self.P = P
        self.front_of = np.zeros(P.n_scalar, dtype=np.int64)
        for s in range(P.n_fronts):
            self.front_of[P.piv0[s]:P.piv0[s] + P.npiv[s]] = s

    def place(self, u, v):
        """(front, row of max, row of min) of Sigma(u, v), or None outside the pattern of L"""
        P = self.P
        lo, hi = min(u, v), max(u, v)
        s = int(self.front_of[lo])
        if hi < P.piv0[s] + P.npiv[s]:
            rh = hi - P.piv0[s]
        else:
            b = P.bnd_rows[P.bnd_off[s]:P.bnd_off[s] + P.nbnd[s]]
            i = int(np.searchsorted(b, hi))
            if i >= len(b) or b[i] != hi:
                return None
            rh = int(P.npiv[s]) + i
        return s, rh, lo - int(P.piv0[s])


def block(rows, Sig, ga, na, gb, nb):
    """Sigma(a, b) from the images; zeros when a vertex is fixed (gidx < 0); None outside the pattern"""
    out = np.zeros((na, nb))
    if ga < 0 or gb < 0:
        return out
    for r in range(na):
        for c in range(nb):
            p = rows.place(ga + r, gb + c)
            if p is None:
                return None
            out[r, c] = Sig[p[0]][p[1], p[2]]
    return out


def dense_system(og):
    """(H dense symmetric, oracle offset per pose, per landmark) of an oracle graph at its current estimates"""
    n, colptr, rowind, values, _ = og.build_system()
    H = np.zeros((n, n))
    for c in range(n):
        for k in range(colptr[c], colptr[c + 1]):
            H[rowind[k], c] = values[k]; H[c, rowind[k]] = values[k]
    po_ = np.zeros(og.n_poses, dtype=np.int32); lo_ = np.zeros(og.n_landmarks, dtype=np.int32)
    assert og.L.orc_vertex_offsets(og.g, _i(po_), _i(lo_)) == n
    return H, po_, lo_


def reference_blocks(Hinv, po_, lo_, g):
    """the blocks gs_compute_marginals reports, cut out of a dense inverse (oracle offsets; fixed vertices: zeros)"""
    def blk(oa, na, ob, nb):
        return np.zeros((na, nb)) if oa < 0 or ob < 0 else Hinv[oa:oa + na, ob:ob + nb]
    poses = np.array([blk(o, 3, o, 3) for o in po_])
    lms = np.array([blk(o, 2, o, 2) for o in lo_])
    pp = np.array([blk(po_[i], 3, po_[j], 3) for i, j in zip(g["pp_i"], g["pp_j"])]).reshape(-1, 3, 3)
    pl = np.array([blk(po_[p], 3, lo_[l], 2) for p, l in zip(g["pl_p"], g["pl_l"])]).reshape(-1, 3, 2)
    return poses, lms, pp, pl


def replay_blocks(P, Sig, g):
    """the same four arrays out of the replayed images (what the host's extraction tables address)"""
    rows = Rows(P)
    pg, lg = P.pose_gidx, P.lm_gidx
    poses = np.array([block(rows, Sig, int(x), 3, int(x), 3) for x in pg])
    lms = np.array([block(rows, Sig, int(x), 2, int(x), 2) for x in lg])
    pp = np.array([block(rows, Sig, int(pg[i]), 3, int(pg[j]), 3) for i, j in zip(g["pp_i"], g["pp_j"])]).reshape(-1, 3, 3)
    pl = np.array([block(rows, Sig, int(pg[p]), 3, int(lg[l]), 2) for p, l in zip(g["pl_p"], g["pl_l"])]).reshape(-1, 3, 2)
    return poses, lms, pp, pl
