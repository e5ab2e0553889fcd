"""Checker of gs_multiply_hessian (numpy): y = H v block by block, in vertex order.

H comes as the six arrays of Graph.export_system() or of the oracle's linearize_blocks() (vertex arrays in insertion order, edge arrays in
insertion order): Hpp_diag [N, 9], Hll_diag [M, 4], Hpp_off [Epp, 9] = the block of (i, j), rows of i, Hpl [Epl, 6] = the block of (pose,
landmark), 3 x 2 row-major.  The graph dict names the endpoints and the fixed vertices.  Rows and columns of fixed vertices are zero
whatever the arrays hold there: y is 0 on them and v is not read on them.

The sums run in numpy's extended precision (np.longdouble) so that the reference's own rounding stays far below the bound it serves:
per component i,  |got_i - ref_i| <= 2 (n_i + 2) 2^-53 (|H| |v|)_i,  n_i = the products in row i (counted here).  A sum of n products has
at most n roundings of a product and n - 1 of an addition, each relative 2^-53 of a partial result that |H| |v| bounds: (2 n - 1) u S to
first order; 2 (n + 2) leaves room for the device summing a landmark's diagonal out of its partial slots and for the final store."""
import numpy as np

U = 2.0 ** -53


def masks(g, N, M):
    fp = np.ones(N, dtype=bool); fp[np.asarray(g["fixed_poses"], dtype=np.int64)] = False
    fl = np.ones(M, dtype=bool); fl[np.asarray(g["fixed_landmarks"], dtype=np.int64)] = False
    return fp, fl


def _mul(B, g, vp, vl, ld):
    N, M = len(B["Hpp_diag"]), len(B["Hll_diag"])
    pp_i = np.asarray(g["pp_i"], dtype=np.int64); pp_j = np.asarray(g["pp_j"], dtype=np.int64)
    pl_p = np.asarray(g["pl_p"], dtype=np.int64); pl_l = np.asarray(g["pl_l"], dtype=np.int64)
    D3 = np.asarray(B["Hpp_diag"], dtype=ld).reshape(N, 3, 3); D2 = np.asarray(B["Hll_diag"], dtype=ld).reshape(M, 2, 2)
    O = np.asarray(B["Hpp_off"], dtype=ld).reshape(-1, 3, 3); W = np.asarray(B["Hpl"], dtype=ld).reshape(-1, 3, 2)
    yp = np.einsum("nij,nj->ni", D3, vp); yl = np.einsum("nij,nj->ni", D2, vl)
    np.add.at(yp, pp_i, np.einsum("eij,ej->ei", O, vp[pp_j])); np.add.at(yp, pp_j, np.einsum("eji,ej->ei", O, vp[pp_i]))
    np.add.at(yp, pl_p, np.einsum("eij,ej->ei", W, vl[pl_l])); np.add.at(yl, pl_l, np.einsum("eji,ej->ei", W, vp[pl_p]))
    return yp, yl


def multiply(B, g, v_pose, v_lm):
    """(y_pose [N, 3], y_lm [M, 2], S_pose, S_lm = (|H| |v|) per component, n_pose [N], n_lm [M] = products per row of the vertex)"""
    ld = np.longdouble
    N, M = len(B["Hpp_diag"]), len(B["Hll_diag"])
    fp, fl = masks(g, N, M)
    vp = np.where(fp[:, None], np.asarray(v_pose, dtype=ld).reshape(N, 3), 0); vl = np.where(fl[:, None], np.asarray(v_lm, dtype=ld).reshape(M, 2), 0)
    yp, yl = _mul(B, g, vp, vl, ld)
    Sp, Sl = _mul({k: np.abs(np.asarray(B[k])) for k in ("Hpp_diag", "Hll_diag", "Hpp_off", "Hpl")}, g, np.abs(vp), np.abs(vl), ld)
    yp[~fp] = 0; yl[~fl] = 0; Sp[~fp] = 0; Sl[~fl] = 0
    n_pose = 3 + 3 * (np.bincount(np.asarray(g["pp_i"], dtype=np.int64), minlength=N) + np.bincount(np.asarray(g["pp_j"], dtype=np.int64), minlength=N)) \
        + 2 * np.bincount(np.asarray(g["pl_p"], dtype=np.int64), minlength=N)
    n_lm = 2 + 3 * np.bincount(np.asarray(g["pl_l"], dtype=np.int64), minlength=M)
    return yp.astype(np.float64), yl.astype(np.float64), Sp.astype(np.float64), Sl.astype(np.float64), n_pose, n_lm


def bound(S_pose, S_lm, n_pose, n_lm):
    """the per-component rounding bound 2 (n_i + 2) u (|H| |v|)_i"""
    return 2.0 * (n_pose[:, None] + 2) * U * S_pose, 2.0 * (n_lm[:, None] + 2) * U * S_lm


def check(got_pose, got_lm, B, g, v_pose, v_lm, extra=0.0):
    """asserts the bound (+ extra, absolute) on every component and exact zeros on fixed vertices; returns the worst err / bound"""
    yp, yl, Sp, Sl, n_p, n_l = multiply(B, g, v_pose, v_lm)
    bp, bl = bound(Sp, Sl, n_p, n_l)
    fp, fl = masks(g, len(yp), len(yl))
    assert not np.asarray(got_pose)[~fp].any() and not np.asarray(got_lm)[~fl].any(), "a fixed vertex's row is not exactly zero"
    ep, el = np.abs(got_pose - yp), np.abs(got_lm - yl)
    worst = 0.0
    for name, e, b in (("pose", ep, bp + extra), ("landmark", el, bl + extra)):
        bad = np.argwhere(e > b)
        assert len(bad) == 0, "%s %s: |err| %.3e > bound %.3e" % (name, bad[0], e[tuple(bad[0])], b[tuple(bad[0])])
        nz = b > 0
        if nz.any():
            worst = max(worst, float((e[nz] / b[nz]).max()))
        assert not e[~nz].any()
    return worst
