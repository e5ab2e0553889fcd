"""What the CPU census and the GPU tests of the grown-plan cases (tests/tail_shapes.py) share (TEST-ONLY): the mpmath reference of a case,
computed once per process, and the two-sided half of the bound with the perturbed term taken from the TAIL.

lin_exact_ref.linearize adds an entry's terms in a fixed order — the odometry edges in index order, then the observation edges in index
order — so term j of an entry of a vertex's block belongs to the j-th edge of that list at the vertex (edges_at): that is how a term is
known to be a tail edge's.  perturbed_fails multiplies ONE qualifying term of ONE entry by (1 + 1e-9) in the reference and asserts that
the unperturbed result then violates the bound there; among the entries where any fp64 evaluation could tell (1e-9 |term| > 2 C u S) it
takes the one with the largest S, and returns None where there is none."""
import numpy as np

import lin_exact_ref as lx
import tail_shapes as ts

_exact = {}


def exact(name):
    """the reference of a case's full graph at its own estimates (tail_shapes.graph(name, ...) has built the case)"""
    if name not in _exact:
        _, _, full, kernels = ts._built[name]
        _exact[name] = lx.linearize(full, kernels)
    return _exact[name]


def edges_at(g, kind, v):
    """[(edge kind, edge index)] in the order lin_exact_ref.linearize adds their terms to the diagonal block and rhs of a FREE vertex"""
    if kind == "pose":
        return [("pp", int(k)) for k in np.flatnonzero((np.asarray(g["pp_i"]) == v) | (np.asarray(g["pp_j"]) == v))] + \
               [("pl", int(k)) for k in np.flatnonzero(np.asarray(g["pl_p"]) == v)]
    return [("pl", int(k)) for k in np.flatnonzero(np.asarray(g["pl_l"]) == v)]


def perturbed_fails(X, blocks, arr, rows, qualifies, tag):
    """rows: block rows of `arr` (vertices or edges); qualifies(row, j): may term j of that row's entries be the perturbed one?
    (flat index, perturbed err / (u S), C) or None"""
    w = lx.WIDTH[arr]; c = X.bound(arr); best = None
    for row in rows:
        for q in range(w):
            idx = int(row) * w + q
            for j, t in enumerate(X.terms[arr].get(idx, ())):
                if qualifies(int(row), j) and lx.REL * float(abs(t)) > 2 * c[idx] * lx.U * X.S[arr][idx] and (best is None or X.S[arr][idx] > X.S[arr][best[0]]):
                    best = (idx, t)
    if best is None:
        return None
    idx, t = best
    got = lx.mpf(float(np.asarray(blocks[arr], dtype=np.float64).reshape(-1)[idx]))
    r = float(abs(got - (X.val[arr][idx] + lx.REL * t))) / (lx.U * X.S[arr][idx])
    assert r > c[idx], (tag, arr, idx, "a tail term off by 1e-9 stays inside the bound", r, float(c[idx]))
    return idx, r, float(c[idx])


def tail_targets(name):
    """the vertices whose diagonal block and rhs a tail term is perturbed in: {label: (kind, vertex)} — the last tail pose that has an
    observation, the last tail cone (where the case has one), the old poses at the older end of a tail odometry edge (the last old pose;
    tail_mixed: pose 30 too), the old free cone the most tail edges touch (tail_mixed: A)"""
    base, tail, full, _ = ts._built[name]
    N0, M0, Epp0, Epl0 = len(base["pose_est"]), len(base["lm_est"]), len(base["pp_i"]), len(base["pl_p"])
    pf = np.zeros(len(full["pose_est"]), dtype=bool); pf[np.asarray(full["fixed_poses"], dtype=np.int64)] = True
    lf = np.zeros(len(full["lm_est"]), dtype=bool); lf[np.asarray(full["fixed_landmarks"], dtype=np.int64)] = True
    out = {"tail pose": ("pose", int(full["pl_p"][Epl0:].max()))}
    if len(full["lm_est"]) > M0:
        out["tail cone"] = ("landmark", len(full["lm_est"]) - 1)
    older = np.minimum(full["pp_i"][Epp0:], full["pp_j"][Epp0:]); older = older[(older < N0) & ~pf[older]]
    for p in sorted(set(int(v) for v in older), reverse=True):
        out["old pose %d" % p] = ("pose", p)
    old = full["pl_l"][Epl0:]; old = old[(old < M0) & ~lf[old]]
    cone = int(np.argmax(np.bincount(old)))
    out["old cone %d" % cone] = ("landmark", cone)
    return out


def check_can_fail_in_the_tail(X, blocks, name, tag, fitted=False):
    """the two-sided half with a TAIL edge's term off by 1e-9, in every array the tail writes or adds to:
      H_pl, H_pp_off        a tail edge's own block (one term: the edge's), in t_Hpl / t_Hpp_off;
      H_pp, b_pose          of a tail pose (t_Hpp_diag / t_b_pose) and of the old poses that get a tail odometry share (the += into base storage);
      H_ll, b_lm            of a tail cone (t_Hll_diag / t_b_lm) and of an old cone that gets tail shares (the += into its first partial-sum slot).
    In the old vertices' entries only the terms of TAIL edges qualify.  Every H entry must have a place where 1e-9 shows; a b entry too,
    unless the case lies at kilometre coordinates or has a robust kernel (lin_exact_ref.assert_two_sided says why), or the old pose's only
    tail edge is an odometry edge of the bench track, whose residual is zero in exact arithmetic at the initial estimates (tail_wg), or
    the estimates are those an update chose (fitted: a term of b is a residual, which the step made small against its S, as in
    test_gpu_side_exact.py's "after update" rows).  The reference alone decides where 1e-9 can show, never the result under test.
    Returns {label: (flat index, perturbed err / (u S), C) or None}."""
    base, tail, full, _ = ts._built[name]; c = ts.CASES[name]
    Epp0, Epl0 = len(base["pp_i"]), len(base["pl_p"])
    first = {"pp": Epp0, "pl": Epl0}
    out = {"Hpl": perturbed_fails(X, blocks, "Hpl", range(Epl0, len(full["pl_p"])), lambda r, j: True, tag),
           "Hpp_off": perturbed_fails(X, blocks, "Hpp_off", range(Epp0, len(full["pp_i"])), lambda r, j: True, tag)}
    for label, (kind, v) in tail_targets(name).items():
        edges = edges_at(full, kind, v)
        is_tail = [k >= first[ek] for ek, k in edges]
        assert any(is_tail), (tag, label, "no tail edge at this vertex")
        for arr in (("Hpp_diag", "b_pose") if kind == "pose" else ("Hll_diag", "b_lm")):
            w = lx.WIDTH[arr]
            assert all(len(X.terms[arr].get(v * w + q, ())) == len(edges) for q in range(w)), (tag, label, arr, "the terms are not one per edge")
            out["%s %s" % (label, arr)] = perturbed_fails(X, blocks, arr, [v], lambda r, j: is_tail[j], tag)
    for k, v in out.items():
        zero_residual = c["wg"] and k.startswith("old pose")       # the track's odometry measurements ARE the differences of its initial poses: the edge's b term is rounding only
        assert v is not None or (k.split()[-1].startswith("b_") and (c["far"] or c["robust"] or zero_residual or fitted)), (tag, k, "1e-9 of a tail term can show nowhere")
    return out


def show(out):
    return " ".join("%s %s" % (k, "-" if v is None else "%.3g" % v[1]) for k, v in out.items())
