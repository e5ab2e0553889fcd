"""CPU tests of the conditioning-free references (tests/exact_ref.py) against exact rational arithmetic, and the census of the front
shapes that tests/test_gpu_exact.py runs (tests/shape_graphs.py), with a numpy replay of every generated plan under the same bounds."""
from fractions import Fraction

import numpy as np
import pytest

from conftest import make_oracle_graph, random_graph
import exact_ref as xr
from plan_exec import Plan
import selinv_exec as sx
import shape_graphs as sg

U = xr.U


def _spanning(rng, n):
    """values of random sign spanning 1e-8 .. 1e8"""
    return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-8, 8, n)


def _exact_residual(H, x, b):
    r = [Fraction(0)] * H.n
    for i, j, v in zip(H.rows, H.cols, H.vals):
        r[i] += Fraction(float(v)) * Fraction(float(x[j]))
    return [r[i] - Fraction(float(b[i])) for i in range(H.n)]


@pytest.mark.parametrize("seed", range(6))
def test_double_double_residual_equals_rational_arithmetic(seed):
    rng = np.random.default_rng(seed)
    n, nnz = 12, 90
    rows = rng.integers(0, n, nnz); cols = rng.integers(0, n, nnz)
    rows = np.concatenate([rows, rows[:10]]); cols = np.concatenate([cols, cols[:10]])          # duplicate entries
    H = xr.Sparse(rows, cols, _spanning(rng, len(rows)), n)
    x = _spanning(rng, n)
    naive = np.zeros(n); np.add.at(naive, rows, H.vals * x[cols])
    b = np.where(np.arange(n) % 2 == 0, naive, _spanning(rng, n))                                # even rows: catastrophic cancellation
    r = H.residual(x, b)
    for got, ex in zip(r, _exact_residual(H, x, b)):
        assert abs(Fraction(float(got)) - ex) <= Fraction(U) * abs(ex) * Fraction(1000001, 1000000), (float(got), float(ex))
    # several right-hand sides at once: the same rows, column by column
    X = np.stack([x, -x, x * 3.0], 1); Bm = np.stack([b, -b, b], 1)
    R = H.residual(X, Bm)
    assert np.array_equal(R[:, 0], r) and np.array_equal(R[:, 1], -r)
    for got, ex in zip(R[:, 2], _exact_residual(H, 3.0 * x, b)):
        assert abs(Fraction(float(got)) - ex) <= Fraction(U) * abs(ex) * Fraction(1000001, 1000000)


def _frac_inverse(A):
    n = len(A)
    M = [[Fraction(float(A[i, j])) for j in range(n)] + [Fraction(int(i == j)) for j in range(n)] for i in range(n)]
    for c in range(n):
        p = max(range(c, n), key=lambda r: abs(M[r][c]))
        M[c], M[p] = M[p], M[c]
        inv = 1 / M[c][c]
        M[c] = [v * inv for v in M[c]]
        for r in range(n):
            if r != c and M[r][c]:
                f = M[r][c]
                M[r] = [a - f * b for a, b in zip(M[r], M[c])]
    return [row[n:] for row in M]


def _dense_sparse(A):
    n = len(A); i, j = np.nonzero(np.ones_like(A))
    return xr.Sparse(i, j, A[i, j], n)


def test_refined_inverse_of_an_ill_conditioned_matrix_is_exact_to_a_few_ulps():
    n = 12
    A = 1.0 / (np.arange(n)[:, None] + np.arange(n)[None, :] + 1.0) + 1.8e-12 * np.eye(n)     # Hilbert + shift: cond ~ 1e12
    assert 1e11 < np.linalg.cond(A) < 1e13
    H = _dense_sparse(A)
    X, X0 = xr.refined_inverse(H, steps=3)
    Xe = _frac_inverse(A)
    worst = max(abs(Fraction(float(X[i, j])) - Xe[i][j]) / abs(Xe[i][j]) for i in range(n) for j in range(n))
    worst0 = max(abs(Fraction(float(X0[i, j])) - Xe[i][j]) / abs(Xe[i][j]) for i in range(n) for j in range(n))
    assert worst < 4 * U, float(worst / U)
    assert worst0 > 1e-8                                                   # the unrefined inverse is nowhere near
    # the bound B = |Sigma| |H| |Sigma| is never below |Sigma|
    B = xr.sigma_bound(H, X0, np.arange(n))
    assert np.all(B >= np.abs(X) * (1 - 1e-12))


def _frac_solve(A, b):
    Ai = _frac_inverse(A)
    return [sum(Ai[i][j] * Fraction(float(b[j])) for j in range(len(b))) for i in range(len(b))]


def test_backward_error_of_the_rounded_exact_solution_and_its_sensitivity():
    rng = np.random.default_rng(4)
    n = 10
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    A = (Q * np.geomspace(1, 50, n)) @ Q.T; A = (A + A.T) / 2
    b = rng.normal(size=n)
    H = _dense_sparse(A)
    x = np.array([float(v) for v in _frac_solve(A, b)])                   # the correctly rounded exact solution
    w = xr.backward_error(H, x, b)
    assert w <= 2 * U, w / U
    k = int(np.argmax(np.abs(x)))
    y = x.copy(); y[k] *= 1 + 1e-9
    assert xr.backward_error(H, y, b) > 1e-12
    # a row with nothing in it (0 / 0) counts as 0
    Z = xr.Sparse([0], [0], [2.0], 2)
    assert xr.backward_error(Z, np.array([0.5, 0.0]), np.array([1.0, 0.0])) == 0.0
    assert xr.backward_error(Z, np.array([0.5, 0.0]), np.array([1.0, 1e-300])) == 1.0


def host_plan(pkg, g, **kw):
    G = pkg.Graph(device=-2, **kw); G.load_bench_graph(g); G.plan_build_host()
    P = Plan(G.plan_export()); G.close()
    P.check_invariants()
    return P


def test_block_system_assembles_the_oracles_scalar_system(pkg, po):
    """the block arrays scattered into the plan's numbering give the oracle's scalar H (duplicate edges, fixed vertices dropped)"""
    g = random_graph(7, n_poses=60, n_lms=30)
    g["fixed_poses"] = np.array([0, 17, 41], dtype=np.int32); g["fixed_landmarks"] = np.array([3, 11], dtype=np.int32)
    P = host_plan(pkg, g)
    og = make_oracle_graph(po, g)
    S = xr.BlockSystem(og.linearize_blocks(), g, P.pose_gidx, P.lm_gidx)
    Ho, po_, lo_ = sx.dense_system(og)
    perm = np.zeros(S.n, dtype=np.int64)                                   # plan scalar -> oracle scalar
    for gp, go, w in ((P.pose_gidx, po_, 3), (P.lm_gidx, lo_, 2)):
        for t in range(w):
            perm[gp[gp >= 0] + t] = go[gp >= 0] + t
    assert S.n == len(Ho)
    Hd = S.H.dense()
    assert np.allclose(Hd, Ho[np.ix_(perm, perm)], rtol=1e-14, atol=1e-14 * np.abs(Ho).max())


def _census_plans(pkg, frontend, bench_graphs):
    plans = []
    for name, (mk, variants) in sg.CASES.items():
        plans.append((name, host_plan(pkg, mk()), variants))
    for name, (mk, variants) in sg.bench_cases(pkg, frontend, bench_graphs).items():
        g = mk()
        plans.append((name, host_plan(pkg, g), variants))
    return plans


def test_census_of_the_front_shapes_the_exact_tests_reach(pkg, frontend, bench_graphs):
    plans = _census_plans(pkg, frontend, bench_graphs)
    hit = sg.census(plans)
    print()
    for name, P, variants in plans:
        f = P.npiv + P.nbnd
        print("%-16s variants %-6s fronts %5d  max f %3d  shapes %s" % (name, variants, P.n_fronts, f.max(),
                                                                     sorted(set(zip(P.npiv.tolist(), P.nbnd.tolist())))[:6]))
    for cell, names in hit.items():
        print("%-40s %3d  %s" % (cell, len(names), ", ".join(names[:6])))
    missing = [c for c, names in hit.items() if not names]
    assert not missing, missing
    # the generators sit where their names say
    fmax = {name: int((P.npiv + P.nbnd).max()) for name, P, _ in plans}
    assert fmax["clique21"] == 63 and fmax["clique20_2lm"] == 64 and fmax["clique53"] == 159 and fmax["clique53_1lm"] in (160, 161)


@pytest.mark.parametrize("name", list(sg.CASES))
def test_replayed_plans_meet_the_exact_bounds(pkg, po, name):
    """plan_exec / selinv_exec replay the plan in numpy: the increment's backward error and Sigma's componentwise error are under the
    bounds the GPU tests use (64 (f_max + 2) u), against the double-double residual and the refined inverse"""
    g = sg.CASES[name][0]()
    P = host_plan(pkg, g)
    fmax = int((P.npiv + P.nbnd).max()); C = 64 * (fmax + 2)
    og = make_oracle_graph(po, g)
    blocks = og.linearize_blocks()
    S = xr.BlockSystem(blocks, g, P.pose_gidx, P.lm_gidx)
    dp, dl, ok = P.solve(blocks)
    assert ok
    w = S.omega(dp, dl)
    assert w <= C * U, (w / U, C)
    Ls, ok = sx.factor(P, blocks)
    Sig = sx.selinv(P, Ls)
    X, X0 = xr.refined_inverse(S.H)
    B = xr.sigma_bound(S.H, X0, np.arange(S.n))
    got = sx.replay_blocks(P, Sig, g)
    ref = sx.reference_blocks(X, P.pose_gidx, P.lm_gidx, g)
    Bb = sx.reference_blocks(B, P.pose_gidx, P.lm_gidx, g)
    worst = 0.0
    for a, r, bb in zip(got, ref, Bb):
        e = np.abs(a - r)
        assert np.all(e <= C * U * bb), float((e / np.maximum(bb, 1e-300)).max() / U)
        if e.size:
            worst = max(worst, float((e / np.maximum(bb, 1e-300)).max() / U))
    print("%s: f_max %d, omega %.2f u, max err / (u B) %.2f, bound %d" % (name, fmax, w / U, worst, C))
