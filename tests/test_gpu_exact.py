"""GPU tests of the solver and the selected inversion against bounds that do not depend on the conditioning of the system.

The parity tests (A8, test_gpu_marginals.py) compare against another fp64 solve, so their tolerances follow cond(H) (7e7 at 1k/200)
and cannot see an error of 1e-10 .. 1e-7 relative.  Here the device's own H, b (gs_export_system) and its own increment are checked
with the references of tests/exact_ref.py:

  solver     omega(dx) = max_i |H dx - b|_i / (|H| |dx| + |b|)_i  <=  64 (f_max + 2) u      (double-double residual)
             and the increment with its largest component times (1 + 1e-9) must exceed that bound;
  marginals  |Sigma_gpu - Sigma_ref|_ij  <=  64 (f_max + 2) u B_ij,   B = |Sigma| |H| |Sigma|  on every entry of every block the four
             getters return (Sigma_ref: the inverse refined in double-double; above 1 600 scalars, sampled columns);

f_max = the plan's largest front, u = 2^-53: 4.6e-13 at f = 63, 1.2e-12 at f = 161.

Measured on the MI355X (omega / u of the step; max err / (u B) of Sigma; the bound C = 64 (f_max + 2) for both):
  graph            f_max   variant 3           variant 4           C        the increment perturbed by 1e-9: ~4e6 u everywhere
  clique21           63    1.87 / 0.50         3.13 / 0.44         4160
  clique20_2lm       64    2.18 / 0.49         2.06 / 0.71         4224
  clique21_1lm       65    2.23 / 0.43         1.89 / 0.52         4288
  clique53          159    4.06 / 0.29         3.54 / 0.33        10304
  clique53_1lm      161        -               3.08 / 0.38        10432
  clique32           96    2.46 / 0.48         2.97 / 0.31         6272
  clique16_chains    59    2.55 / 0.31         2.40 / 0.28         3904
  forest             26    2.10 / 0.55         2.38 / 0.40         1792
  bench 50/30        44    4.00 / 0.08         3.66 / 0.15         2944
  bench 1k/200       57    4.86 / 0.06         11.1 / 0.08         3776     (Sigma: sampled columns)
  track400 K=16     101    6.24 / 0.10             -               6592
  track400 K=24     146    8.67 / 0.06             -               9472
  random80 (v4)     268        -               6.38 / 0.46        17280
  growth 1k K=16    101    4.54 / 0.05             -               6592     (Sigma: sampled columns)
  cfg3 launch modes  57    44.7 (every mode)                       3776
  cfg3 steps 1, 10   57    44.7, 69.1                              3776
  cfg4 steps 1, 10   57    382, 529                                3776
"""
import numpy as np
import pytest

from conftest import append_tail, split_for_growth
import exact_ref as xr
import lin_exact_ref as lx
from plan_exec import Plan
import selinv_exec as sx
import shape_graphs as sg

pytestmark = pytest.mark.gpu
U = xr.U
DENSE_MAX = 1600                                         # scalars: every column of Sigma refined up to here, sampled columns beyond


def fresh(pkg, g, debug=None, **kw):
    G = pkg.Graph(device=0, debug=debug, **kw)
    G.load_bench_graph(g)
    return G


def plan_of(G):
    P = Plan(G.plan_export())
    fmax = int((P.npiv + P.nbnd).max())
    return P, fmax, 64 * (fmax + 2)


def check_omega(S, dp, dl, C, tag):
    """backward error of the increment, and of the increment with its largest component off by 1e-9 relative"""
    w = S.omega(dp, dl)
    x = S.scatter(dp, dl); k = int(np.argmax(np.abs(x)))
    y = x.copy(); y[k] *= 1 + 1e-9
    w2 = xr.backward_error(S.H, y, S.b)
    print("%s: omega %.2f u (bound %d u), perturbed %.3g u" % (tag, w / U, C, w2 / U))
    assert w <= C * U, (tag, w / U, C)
    assert w2 > C * U, (tag, w2 / U, C)
    return w


def device_system(G, g):
    """the H and b of the handle's last linearisation (the last iteration's, or gs_compute_marginals')"""
    P, fmax, C = plan_of(G)
    return xr.BlockSystem(G.export_system(), g, P.pose_gidx, P.lm_gidx), P, fmax, C


def check_step(G, g, tag, iterations=1):
    """the handle's next `iterations` steps; the last one against the H and b it solved"""
    done, st = G.optimize(iterations)
    assert done == iterations and st.numeric_failure == 0
    S, P, fmax, C = device_system(G, g)
    dp, dl = G.export_delta()
    return check_omega(S, dp, dl, C, "%s f_max %d" % (tag, fmax))


def blocks_of(G):
    return G.pose_covariances(), G.landmark_covariances(), G.odometry_edge_covariances(), G.observation_edge_covariances()


def check_sigma(S, P, g, got, C, tag, seed=0):
    """every entry of the four getters' blocks within C u B of the refined inverse (columns of a sample of vertices above DENSE_MAX
    scalars: a block is checked when one of its two vertices is in the sample)"""
    X0 = np.linalg.inv(S.H.dense()); X0 = (X0 + X0.T) / 2
    pg, lg = P.pose_gidx, P.lm_gidx
    if S.n <= DENSE_MAX:
        cols = np.arange(S.n)
    else:
        rng = np.random.default_rng(seed)
        ps = rng.choice(pg[pg >= 0], min(96, int((pg >= 0).sum())), replace=False)
        ls = rng.choice(lg[lg >= 0], min(48, int((lg >= 0).sum())), replace=False)
        cols = np.unique(np.concatenate([ps[:, None] + np.arange(3), ls[:, None] + np.arange(2)], axis=None))
    X = xr.refine_columns(S.H, cols, X0)
    B = xr.sigma_bound(S.H, X0, cols)
    Xf = np.full((S.n, S.n), np.nan); Bf = np.full((S.n, S.n), np.nan)
    Xf[:, cols] = X; Xf[cols, :] = X.T; Bf[:, cols] = B; Bf[cols, :] = B.T       # Sigma and B are symmetric
    ref = sx.reference_blocks(Xf, pg, lg, g); Bb = sx.reference_blocks(Bf, pg, lg, g)
    worst, checked = 0.0, 0
    for name, a, r, bb in zip(("poses", "landmarks", "odometry edges", "observation edges"), got, ref, Bb):
        if not len(a):
            continue
        assert a.shape == r.shape, name
        m = np.isfinite(r)
        e = np.abs(a - r)[m]; bb = bb[m]
        checked += int(m.sum())
        assert np.all(e <= C * U * bb), (tag, name, float((e / np.maximum(bb, 1e-300)).max() / U), C)
        if e.size:
            worst = max(worst, float((e / np.maximum(bb, 1e-300)).max() / U))
    assert checked >= min(S.n, 200), checked
    print("%s: Sigma max err / (u B) %.2f (bound %d), %d entries, %s" % (tag, worst, C, checked, "dense" if S.n <= DENSE_MAX else "sampled"))
    return worst


def check_marginals(G, g, tag):
    info = G.compute_marginals()
    assert info["numeric_failure"] == 0
    S, P, fmax, C = device_system(G, g)                             # the marginals call is a linearisation: the H it inverted
    return check_sigma(S, P, g, blocks_of(G), C, "%s f_max %d" % (tag, fmax))


def run_both(pkg, g, variant, tag):
    G = fresh(pkg, g, factor_variant=variant)
    check_step(G, g, "%s v%d step 1" % (tag, variant))
    P, fmax, _ = plan_of(G)
    assert G.stats().factor_variant == (4 if fmax > 159 else variant), (G.stats().factor_variant, fmax)
    check_marginals(G, g, "%s v%d" % (tag, variant))
    G.close()


@pytest.mark.parametrize("name,variant", [(n, v) for n, (_, vs) in sg.CASES.items() for v in vs])
def test_shape_graphs(pkg, name, variant):
    run_both(pkg, sg.CASES[name][0](), variant, name)


@pytest.mark.parametrize("name,variant", [(n, v) for n, vs in sg.BENCH_VARIANTS.items() for v in vs])
def test_bench_tracks_and_random_graphs(pkg, frontend, bench_graphs, name, variant):
    run_both(pkg, sg.bench_cases(pkg, frontend, bench_graphs)[name][0](), variant, name)


@pytest.mark.parametrize("name", ["clique20_2lm", "bench1k"])
def test_the_export_holds_the_last_linearisation(pkg, frontend, bench_graphs, name):
    """gs_export_system returns the H and b of the last linearisation whichever call ran it: an iteration of gs_optimize (the estimates
    before its update) and gs_compute_marginals give, bit for bit, what gs_linearize gives at the same estimates — the landmark blocks
    too, which those calls keep as per-edge partials that only the fronts sum"""
    g = sg.CASES[name][0]() if name in sg.CASES else sg.bench_cases(pkg, frontend, bench_graphs)[name][0]()
    G = fresh(pkg, g)
    G.linearize(); before = G.export_system()
    done, st = G.optimize(1); assert done == 1
    after_step = G.export_system()
    G.linearize(); moved = G.export_system()
    G.compute_marginals(); after_marginals = G.export_system()
    for k in before:
        assert np.array_equal(after_step[k], before[k]), k
        assert np.array_equal(after_marginals[k], moved[k]), k
    assert not np.array_equal(moved["Hll_diag"], before["Hll_diag"]) and not np.array_equal(moved["b_lm"], before["b_lm"])
    G.close()


@pytest.mark.parametrize("env", [dict(tree=0), dict(leaf_kernel=0), dict(leaf_kernel=2), dict(block_fronts=0),
                                 dict(leaf_kernel=2, subtree=1, block_fronts=0), dict(tickets=1)])
def test_solver_launch_modes(pkg, bench_graphs, env):
    """the launch modes of test_solver_launch_modes_give_the_same_answer, on its 10k / 2k graph"""
    _, g = bench_graphs(10000, 2000)
    G = fresh(pkg, g, debug=env)
    check_step(G, g, "cfg3 %s" % env)
    G.close()


def test_growth_across_the_wave_workgroup_split(pkg, frontend):
    """K = 16 track of 1 000 poses, three appended keyframes: fronts of 61 and 63 scalars grow to 64 and 72 (a wave front becomes a
    workgroup front).  H and b are the grown handle's own export (tail arenas and the tail's shares in base storage); a fresh handle of
    the whole graph linearised at the grown handle's estimates is the cross-check: the two systems agree entry by entry within twice the
    linearisation bound 2 (34 + n) u S (each is within it of the exact system; S and n from lin_exact_ref.magnitudes, exact zeros where
    S = 0).  test_gpu_tail_exact.py holds both handles to the mpmath reference itself on this track cut to 60 poses."""
    t = pkg.track.generate(1000, 200, 16); g = pkg.track.bench_graph(t, frontend)
    base, tail, full = split_for_growth(g, 3)
    G = fresh(pkg, base); G.optimize(2)
    P0, _, _ = plan_of(G)
    for k in range(3):
        append_tail(G, tail, (k, k + 1)); G.initialize_optimization()
        assert G.plan_growths() == k + 1, G.growth_refusal()
    P, fmax, C = plan_of(G)
    f0, f1 = P0.npiv + P0.nbnd, (P.npiv + P.nbnd)[:P0.n_fronts]
    assert ((f0 <= 63) & (f1 >= 64)).any(), "no front crossed from a wave to a workgroup"

    def system():
        """the grown handle's system at its current estimates (gs_linearize, as the fresh handle below) against a fresh handle's"""
        G.linearize(); own = G.export_system()
        F = fresh(pkg, dict(full, pose_est=G.poses(), lm_est=G.landmarks()))
        F.linearize(); sysm = F.export_system(); F.close()
        Sm, n = lx.magnitudes(full, G.poses(), G.landmarks()); worst = 0.0
        for k in own:
            assert own[k].shape == sysm[k].shape, k
            d = np.abs(own[k] - sysm[k]).reshape(-1); tol = 2 * lx.C(n[k]) * U * Sm[k]
            assert np.all(d <= tol), (k, int(np.argmax(d - tol)), float((d - tol).max()))
            worst = max(worst, float((d[tol > 0] / tol[tol > 0]).max()))
        print("growth: the grown handle's export against a fresh handle's: worst |difference| / (2 C(n) u S) %.4f" % worst)
        return xr.BlockSystem(own, full, P.pose_gidx, P.lm_gidx)
    S = system()
    done, st = G.optimize(1)
    assert done == 1 and st.numeric_failure == 0
    dp, dl = G.export_delta()
    check_omega(S, dp, dl, C, "growth step f_max %d" % fmax)
    S = system()
    info = G.compute_marginals(); assert info["numeric_failure"] == 0
    check_sigma(S, P, full, blocks_of(G), C, "growth f_max %d" % fmax)
    G.close()


@pytest.mark.parametrize("N,M", [(10000, 2000), (100000, 10000)])
def test_large_configurations_solver(pkg, bench_graphs, N, M):
    """cfg3 / cfg4: the backward error of the first and the tenth increment (the sparse double-double residual only)"""
    _, g = bench_graphs(N, M)
    G = fresh(pkg, g)
    check_step(G, g, "%dk step 1" % (N // 1000))
    check_step(G, g, "%dk step 10" % (N // 1000), iterations=9)
    G.close()
