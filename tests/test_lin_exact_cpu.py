"""The linearisation cases, their reference and their bound, checked without a GPU.

  census        every case of tests/lin_shapes.py reaches the path it is named for: the host-only plan has the forced T, the R, the tile
                count, the per-tile landmark-group class and the gather fallback exactly where intended;
  soundness     the unchanged CPU oracle (orc_linearize_blocks, orc_chi2; robust cases: on robust_ref's re-weighted graph) stays inside
                C(n) u S of tests/lin_exact_ref.py on every entry of every case, and a reference with one term off by 1e-9 does not;
  independence  the reference's Jacobians are the central differences of its own error functions.

The oracle's worst err / (u S) per case (largest over the six arrays, chi2 and the per-edge s; the bound's C(n) is at least 70, 144 robust):
  t1_r1              3.56 Hpp_off    t1_r2              3.50 Hpp_off    t1_r3              4.03 Hpp_diag
  t1_r4              3.98 Hpp_diag   t1_tiles3          5.42 Hpp_diag   t1_groups          4.04 Hpp_diag
  t1_groups12        2.80 Hpp_off    t1_groups13to25    3.34 Hpp_off    t2_k2              3.52 Hpp_diag
  t2_k4              3.98 Hpp_diag   t2_k5              3.74 Hpp_diag   t2_k8              3.93 Hpp_off
  t4_k4              5.19 Hpp_diag   t4_k8              4.01 Hpp_diag   t4_k9              4.25 Hpp_off
  t4_k16             4.49 Hpp_diag   t8_k16             3.31 Hpl        t8_k17             3.80 Hpl
  t8_k32             3.95 Hpp_off    auto_k8            3.76 Hpp_off    t1_k5              3.74 Hpp_diag
  t2_k9              3.84 Hpp_off    t4_k17             3.68 Hpp_off    t8_k33             4.55 Hpp_diag
  far_t1             3.22 Hpp_off    far_t2             4.22 Hpp_diag   far_t4             3.31 Hpp_off
  far_t8             3.68 Hpp_off    n_lt_tile          2.72 Hpp_off    robust_t1          3.48 Hpp_diag
  robust_t1_r1       2.45 Hpp_off    robust_t1_r2       3.42 Hpp_off    robust_t1_r4       3.38 Hpp_off
  robust_t2          2.61 Hpp_off    robust_t2_r1       3.28 Hpp_off    robust_t2_r2       3.38 Hpp_off
  robust_t2_r4       3.37 Hpp_off    robust_t4          2.49 Hpp_off    robust_t4_r1       3.92 Hpp_diag
  robust_t4_r2       3.28 Hpp_off    robust_t4_r4       2.78 Hpp_off    robust_t8          2.64 Hpp_diag
  robust_t8_r1       2.89 Hpp_off    robust_t8_r2       3.67 Hpp_off    robust_t8_r4       3.22 Hpp_off
"""
import numpy as np
import pytest

from conftest import make_oracle_graph
import lin_exact_ref as lx
import lin_shapes as ls
from plan_exec import Plan
import robust_ref as rr

_exact = {}


def exact(name):
    if name not in _exact:
        g, kernels, _ = ls.graph(name)
        _exact[name] = lx.linearize(g, kernels)
    return _exact[name]


def tile_groups(P, g, N):
    """distinct landmarks per wave tile, from the plan's own ELL layout: index = slot * (T N) + T pose + lane"""
    T = P.ell_T; PW = 64 // T; tiles = -(-N // PW)
    seen = [set() for _ in range(tiles)]
    for e in np.flatnonzero(P.ell_ins[:-1] >= 0):
        pose = (e % (T * N)) // T
        assert g["pl_p"][P.ell_ins[e]] == pose
        seen[pose // PW].add(int(g["pl_l"][P.ell_ins[e]]))
    return [len(s) for s in seen]


@pytest.mark.parametrize("name", list(ls.CASES))
def test_census(pkg, name):
    c = ls.CASES[name]; g, kernels, notes = ls.graph(name); N = c["N"]
    G = pkg.Graph(device=-2, debug=dict(ell_lanes=c["T"])); G.load_bench_graph(g); G.plan_build_host()
    P = Plan(G.plan_export()); G.close()
    T = c["T"] or 8; PW = 64 // T; tiles = -(-N // PW)
    assert (P.ell_T, P.ell_R) == (T, c["R"]), (P.ell_T, P.ell_R)
    assert (P.ell_R > ls.LIN_R) == c["fallback"] == (name in ("t1_k5", "t2_k9", "t4_k17", "t8_k33"))
    assert P.ell_len == P.ell_R * T * N + 1
    assert N % PW != 0 and N - (tiles - 1) * PW == (5 if N == 5 else 6), "the last tile is to have 6 live poses"
    assert tiles == (1 if N == 5 else {1: 2, 2: 3, 4: 5, 8: 9}[T] + (1 if N == 134 else 0))
    counts = np.bincount(g["pl_p"], minlength=N)
    assert counts.max() == c["kmax"] and counts[0] >= 1 and (counts == 0).any()
    assert np.array_equal(counts, notes["counts"])
    if not c["fallback"]:                                          # every slot holds an edge somewhere, every slot but the last in every lane
        used = np.zeros((P.ell_R, T), dtype=bool)
        for e in np.flatnonzero(P.ell_ins[:-1] >= 0):
            used[e // (T * N), e % T] = True
        assert used.any(axis=1).all() and used[:-1].all(), used
    ng = tile_groups(P, g, N)
    if c["groups"] == "loop":
        assert ng[0] > 25, ng
    elif c["groups"] == "first":
        assert max(ng) <= 12 and ng[0] >= 1, ng
    elif c["groups"] == "both":
        assert 13 <= ng[0] <= 25 and max(ng) <= 25, ng
    # what every graph has
    assert list(g["fixed_poses"]) == [0] and len(g["fixed_landmarks"]) == 1
    F = int(g["fixed_landmarks"][0])
    assert ((g["pl_p"] == 0) & (g["pl_l"] == F)).sum() == 1, "the edge with both ends fixed"
    assert ((g["pl_p"] != 0) & (g["pl_l"] == F)).any(), "the fixed landmark seen from a free pose"
    pairs = g["pl_p"].astype(np.int64) * 100000 + g["pl_l"]
    assert (len(np.unique(pairs)) < len(pairs)) == (c["kmax"] >= 2), "one duplicated pose-landmark edge"
    inc = np.bincount(np.concatenate([g["pp_i"], g["pp_j"]]), minlength=N)
    assert inc[notes["hub"]] == max(5, T + 1) == inc.max() and inc.max() > T
    wide_tiles = {int(p) // PW for p in g["pl_p"][g["pl_l"] == notes["wide"]]}
    assert len(wide_tiles) >= min(3, tiles), wide_tiles
    for W in (np.asarray(g["pl_info"]).reshape(-1, 2, 2), np.asarray(g["pp_info"]).reshape(-1, 3, 3)):
        assert np.array_equal(W, W.transpose(0, 2, 1)) and np.abs(W[:, 0, 1]).min() > 0, "anisotropic, exactly symmetric information"
    if c.get("far"):
        assert np.abs(g["pose_est"][:, :2]).min() > 2.9e4
    if c.get("robust"):
        s_pp, s_pl = rr.edge_s(g, g["pose_est"], g["lm_est"])
        d2 = kernels["odometry"][1] ** 2
        assert kernels["odometry"][0] == "huber" and kernels["observation"][0] == "cauchy" and (s_pp > d2).any() and (s_pp < d2).any()


def test_the_planner_can_produce_every_T_and_R_the_cases_cover():
    plain = {(c["T"] or 8, c["R"]) for c in ls.CASES.values() if not c.get("robust") and not c["fallback"]}
    robust = {(c["T"], c["R"]) for c in ls.CASES.values() if c.get("robust")}
    every = {(T, R) for T in (1, 2, 4, 8) for R in (1, 2, 3, 4)}
    assert plain == every and robust == every


@pytest.mark.parametrize("name", list(ls.CASES))
def test_the_oracle_stays_inside_the_bound_and_a_perturbed_reference_does_not(po, name):
    g, kernels, _ = ls.graph(name); X = exact(name)
    gw = rr.reweighted(g, g["pose_est"], g["lm_est"], kernels) if kernels else g
    og = make_oracle_graph(po, gw)
    blocks = og.linearize_blocks()
    chi2 = rr.robust_chi2(g, g["pose_est"], g["lm_est"], kernels) if kernels else og.chi2()
    s_pp, s_pl = rr.edge_s(g, g["pose_est"], g["lm_est"])
    worst = lx.check(X, blocks, chi2, s_pp, s_pl, tag=name)
    moved = lx.check_can_fail(X, blocks, chi2, tag=name)
    print("%-18s oracle err / (u S): %s | perturbed: %s" % (name, " ".join("%s %.2f" % (k, v) for k, v in worst.items()),
          " ".join("%s %s" % (k, "-" if v is None else "%.3g%s" % (v[1], "*" if v[3] else "")) for k, v in moved.items())))
    lx.assert_two_sided(moved, far=bool(ls.CASES[name].get("far")), robust=bool(kernels), tag=name)


def test_the_reference_counts_what_is_summed():
    """n and the fixed-vertex rule on the smallest case: zero rows and columns with n = 0, S = 0; the edge between the fixed pair in no sum"""
    g, _, _ = ls.graph("n_lt_tile"); X = exact("n_lt_tile")
    assert all(v == 0 for v in X.val["Hpp_diag"][:9]) and not X.n["Hpp_diag"][:9].any() and not X.S["b_pose"][:3].any()
    F = int(g["fixed_landmarks"][0])
    assert not X.n["Hll_diag"][4 * F:4 * F + 4].any()
    both = np.flatnonzero((g["pl_p"] == 0) | (g["pl_l"] == F))
    assert not X.n["Hpl"].reshape(-1, 6)[both].any() and X.n["Hpl"].reshape(-1, 6)[np.setdiff1d(np.arange(len(g["pl_p"])), both)].all()
    assert X.chi2_n == len(g["pl_p"]) + len(g["pp_i"]) - 1
    inc = np.bincount(np.concatenate([g["pp_i"], g["pp_j"]]), minlength=5) + np.bincount(g["pl_p"], minlength=5)
    assert np.array_equal(X.n["Hpp_diag"].reshape(-1, 9)[1:, 0], inc[1:])
    assert len(X.s_pl) == len(g["pl_p"]) and len(X.s_pp) == len(g["pp_i"])


def test_reference_jacobians_are_the_central_differences_of_its_errors():
    """two poses, one landmark: d e / d (additive update) by central differences in mpmath, step 1e-20, to 1e-15"""
    mpf = lx.mpf; h = mpf("1e-20")
    xi = [mpf(v) for v in (1.25, -0.5, 0.7)]; xj = [mpf(v) for v in (2.0, 0.25, 1.1)]; l = [mpf(v) for v in (4.5, 2.25)]
    zpp = [mpf(v) for v in (0.9, 0.1, 0.35)]; zpl = [mpf(v) for v in (3.0, 0.5)]

    def fd(f, x, k):
        a = list(x); b = list(x); a[k] += h; b[k] -= h
        return [(p - m) / (2 * h) for p, m in zip(f(a), f(b))]
    A, B = lx.jac_pl(xi, l)
    for k in range(3):
        d = fd(lambda x: lx.err_pl(x, l, zpl), xi, k)
        assert all(abs(d[r] - A[r][k]) < 1e-15 for r in range(2)), (k, d)
    for k in range(2):
        d = fd(lambda x: lx.err_pl(xi, x, zpl), l, k)
        assert all(abs(d[r] - B[r][k]) < 1e-15 for r in range(2)), (k, d)
    A, B = lx.jac_pp(xi, xj, zpp)
    for k in range(3):
        d = fd(lambda x: lx.err_pp(x, xj, zpp), xi, k)
        assert all(abs(d[r] - A[r][k]) < 1e-15 for r in range(3)), (k, d)
        d = fd(lambda x: lx.err_pp(xi, x, zpp), xj, k)
        assert all(abs(d[r] - B[r][k]) < 1e-15 for r in range(3)), (k, d)
    assert any(abs(A[r][2]) > 0.1 for r in range(2))              # the lever arm is there to be wrong


def test_the_bound_refuses_a_wrong_small_entry():
    """what the norm-wise bar cannot see: the smallest non-zero H_pl entry of a case off by 1e-12 relative fails, and passes untouched"""
    X = exact("t2_k5")
    blocks = {k: np.array([float(v) for v in X.val[k]]) for k in lx.ARRAYS}
    lx.check(X, blocks, tag="rounded reference")
    nz = np.flatnonzero(blocks["Hpl"]); k = nz[np.argmin(np.abs(blocks["Hpl"][nz]))]
    assert abs(blocks["Hpl"][k]) < 1e-3 * np.abs(blocks["Hpl"]).max()
    if 1e-12 * abs(blocks["Hpl"][k]) > 2 * lx.C(1) * lx.U * X.S["Hpl"][k]:
        blocks["Hpl"][k] *= 1 + 1e-12
        with pytest.raises(AssertionError):
            lx.check(X, blocks, tag="one small entry off")
    else:
        blocks["Hpl"][k] += 4 * lx.C(1) * lx.U * X.S["Hpl"][k]
        with pytest.raises(AssertionError):
            lx.check(X, blocks, tag="one small entry off")
