"""Powell's dogleg without a GPU: the conditions of test_gpu_dogleg.py established with the checker (dogleg_ref.py: g2o's rule on the CPU
oracle) alone, and the C-ABI surface of gs_optimize_dogleg / gs_multiply_hessian on host-only handles.

The start: x1 of test_lm_cpu.starts(seed 1) — bench 1000 / 200, its oracle optimum perturbed, one oracle Gauss-Newton iteration."""
import ctypes as C

import numpy as np
import pytest

import dogleg_ref as dr
import polar_ref as plr
from test_lm_cpu import BOUNDARY, boundary_start, robust_case, starts

DEFAULT_TRIALS = [4, 1, 1, 1, 1, 1]
DEFAULT_KINDS = ["GN", "GN", "GN", "DL", "DL", "GN", "DL", "GN", "GN"]           # per trial; the first three are rejected
SMALL_KINDS = ["SD", "SD", "SD", "DL", "DL", "DL"]                                # initial_delta = 1, all accepted
SIDE_ITERATIONS = 4
SIDE_TRIALS = [5, 1, 1, 1]
SIDE_INACTIVE = (11, 203)                                                         # two Cartesian observation edges of the side case

_runs = {}


def x1_model(po, bench_graphs):
    g, _, _, P1, L1, _, _ = starts(po, bench_graphs, 1)
    return dr.Model(po, g), P1, L1


def x1_run(po, bench_graphs, which):
    """the three trajectories of the GPU suite from x1, computed once per process: "default" (6 iterations), "small" (initial_delta = 1),
    "terminate" (max_trials = 3)"""
    if which not in _runs:
        m, P1, L1 = x1_model(po, bench_graphs)
        kw = dict(default={}, small=dict(initial_delta=1.0), terminate=dict(max_trials=3))[which]
        _runs[which] = dr.run(m, 6, poses=P1, lms=L1, **kw)
    return _runs[which]


def side_case(po, bench_graphs):
    """(model, graph, x1, kernels, polar set, prior, inactive edges): Huber on the observation kind (robust_case), one pose prior, the
    polar set of polar_ref.polar_set, two inactive Cartesian edges"""
    g, P1, L1, kernels = robust_case(po, bench_graphs)
    polar = plr.polar_set(dict(g, pose_est=P1, lm_est=L1))
    off = tuple(k for k in SIDE_INACTIVE)
    assert not set(off) & set(int(i) for i in polar["idx"])
    rng = np.random.default_rng(5)
    A = rng.normal(size=(3, 3)); W = 0.4 * (A @ A.T + 3 * np.eye(3)); W = (W + W.T) / 2
    pri = dict(pose=[(500, P1[500] + [0.2, -0.1, 0.02], W, False)], lm=[])
    return dr.Model(po, g, kernels=kernels, polar=polar, pri=pri, off=off), g, P1, L1, kernels, polar, pri, off


def side_run(po, bench_graphs):
    if "side" not in _runs:
        m, g, P1, L1 = side_case(po, bench_graphs)[:4]
        _runs["side"] = dr.run(m, SIDE_ITERATIONS, poses=P1, lms=L1)
    return _runs["side"]


def show(label, r):
    mg, rg, bg = dr.figures(r)
    print("%s: trials %s kinds %s\n  chi2 %s -> %.6g, delta[] %s -> %.6g\n  smallest margin %.3g, rho gap %.3g, branch gap %.3g\n%s" % (
        label, r["n_trials"].tolist(), [dr.KINDS[t["kind"]] for t in r["trials"]], np.round(r["chi2"], 1).tolist(), r["chi2_final"],
        ["%.6g" % d for d in r["delta"]], r["delta_final"], mg, rg, bg, dr.describe(r)))


def test_default_parameters_from_x1(po, bench_graphs):
    """Default parameters (initial_delta 1e4, max_trials 100), 6 iterations from x1.  Measured with the committed checker:
    trials per iteration [4, 1, 1, 1, 1, 1]; kinds GN GN GN (rejected, rho -0.2318 each: delta 1e4, 5000, 2500 stay above |h_gn| = 1480.5)
    then DL at delta 1250, DL (625), GN (1875), DL (937.5), GN, GN (2812.5); chi2 at the accepted points 63 935.1 -> 56 369.7 -> 23 913.2
    -> 21 508.4 -> 3 110.7 -> 1 748.8 -> 1 636.05; rho -0.2318 x3, 0.1275, 0.9724, 0.1102, 0.9768, 0.9601, 0.8489; smallest margin 6.45e-2;
    the nearest a rho comes to 0, 0.25 or 0.75 is 0.0989 (0.8489 against 0.75); the closest branch comparison is |h_gn| 1673.5 against
    delta 1875 (0.107 relative)."""
    r = x1_run(po, bench_graphs, "default")
    show("default", r)
    assert r["n_trials"].tolist() == DEFAULT_TRIALS and r["accepted"] == 6 and r["rejected"] == 3 and not r["terminated"]
    assert [dr.KINDS[t["kind"]] for t in r["trials"]] == DEFAULT_KINDS
    assert [t["accepted"] for t in r["trials"]] == [False] * 3 + [True] * 6
    dr.conditions(r)
    assert np.all(np.diff(np.r_[r["chi2"], r["chi2_final"]]) < 0)


def test_small_initial_delta_from_x1(po, bench_graphs):
    """initial_delta = 1, 6 iterations from x1.  Measured: kinds SD SD SD DL DL DL, all accepted, the radius tripling with every step
    (rho 1.01 .. 1.37 > 0.75): delta 1, 3, 9, 27, 81, 243; smallest margin 2.7e-2; the closest branch comparison is delta 27 against
    |h_sd| 25.3 (6.2e-2 relative)."""
    r = x1_run(po, bench_graphs, "small")
    show("initial_delta = 1", r)
    assert r["n_trials"].tolist() == [1] * 6 and r["accepted"] == 6 and r["rejected"] == 0
    assert [dr.KINDS[t["kind"]] for t in r["trials"]] == SMALL_KINDS
    dr.conditions(r)


def test_three_trials_from_x1_terminate(po, bench_graphs):
    """max_trials = 3 with the default initial_delta: the three Gauss-Newton trials of the default run are three rejections (rho -0.2318
    each, margin 0.22), so the call terminates with nothing accepted."""
    r = x1_run(po, bench_graphs, "terminate")
    show("max_trials = 3", r)
    assert r["terminated"] and r["accepted"] == 0 and r["rejected"] == 3 and r["n_trials"].tolist() == [3]
    assert all(t["kind"] == dr.GN and abs(t["rho"] + 0.2318) < 1e-3 for t in r["trials"])
    dr.conditions(r)
    assert r["delta_final"] == 1e4 / 8


def boundary_terminate(po, g, P1, L1):
    """the checker's run from a boundary start (test_lm_cpu.boundary_start) with max_trials = 3 and the default initial_delta; asserted:
    three rejections, "terminate", and dogleg_ref.conditions on every trial"""
    r = dr.run(dr.Model(po, g), 6, poses=P1, lms=L1, max_trials=3)
    assert r["terminated"] and r["accepted"] == 0 and r["rejected"] == 3 and r["n_trials"].tolist() == [3]
    dr.conditions(r)
    return r


@pytest.mark.parametrize("total", sorted(BOUNDARY))
def test_boundary_graphs_terminate_with_the_checker_alone(po, bench_graphs, total):
    """The condition of test_gpu_dogleg.py's terminate-and-restore test at N + M = 255, 256, 257 (one workgroup with an idle thread,
    exactly one, a second one of a single landmark): three rejected trials, every margin, rho gap and branch gap (printed)."""
    g, P1, L1 = boundary_start(po, bench_graphs, total)
    show("N + M = %d" % total, boundary_terminate(po, g, P1, L1))


def test_robust_and_side_pass_case(po, bench_graphs):
    """The case of the GPU suite's robust / side-pass test: Huber on the observation kind (delta = median sqrt(s) at x1), one pose prior,
    polar_ref.polar_set, two inactive edges; 4 iterations from x1 with default parameters.  Measured: trials [5, 1, 1, 1]; kinds GN x4
    (rejected, rho -0.0920 each, delta 1e4 .. 1250 above |h_gn| = 1150.6), DL at delta 625 (rho 0.6939), DL (0.8700), GN (0.7855), GN
    (0.9276); chi2 62 855.9 -> 27 570.4 -> 6 387.1 -> 2 602.9 -> 1 520.57; smallest margin 8.6e-2, rho gap 3.6e-2 (0.7855 against 0.75),
    branch gap 8.0e-2 (|h_gn| 1150.6 against delta 1250).  Asserted: every trial's margin, rho gap and branch gap (dogleg_ref.conditions)."""
    r = side_run(po, bench_graphs)
    show("huber + prior + polar + inactive", r)
    assert r["accepted"] == SIDE_ITERATIONS and not r["terminated"] and r["n_trials"].tolist() == SIDE_TRIALS
    dr.conditions(r)
    assert np.all(np.diff(np.r_[r["chi2"], r["chi2_final"]]) < 0)


def test_checker_pieces(po, bench_graphs):
    """the checker's own sanity: sym_mul against a dense product; a radius below |h_sd| gives the scaled gradient, one above |h_gn| the
    Gauss-Newton step, one between a step of exactly that length"""
    from conftest import make_oracle_graph
    _, g = bench_graphs(50, 30)
    m = dr.Model(po, g)
    og, n, colptr, rowind, values, b = m.system(g["pose_est"], g["lm_est"])
    A = np.zeros((n, n))
    for j in range(n):
        for k in range(colptr[j], colptr[j + 1]):
            A[rowind[k], j] = values[k]; A[j, rowind[k]] = values[k]
    x = np.random.default_rng(0).normal(size=n)
    assert np.abs(dr.sym_mul(n, colptr, rowind, values, x) - A @ x).max() <= 1e-12 * np.abs(A @ x).max()
    gn, sd = dr.first_norms(m)
    assert sd < gn
    pt = dr.Point(m, np.asarray(g["pose_est"], dtype=np.float64), np.asarray(g["lm_est"], dtype=np.float64))
    for delta, kind in ((2 * gn, dr.GN), (0.5 * sd, dr.SD), (0.5 * (gn + sd), dr.DL)):
        h, k, _, _, _ = dr.blend(pt.h_gn, pt.h_sd, delta)
        assert k == kind
        if kind != dr.GN:
            assert abs(np.linalg.norm(h) - delta) <= 1e-12 * delta
    og2 = make_oracle_graph(po, g); og2.build_system(); og2.apply_update(og2.solve_ldlt(1))
    t = dr.trial(m, pt, 2 * gn)
    assert np.abs(t["dpose"] - og2.delta()[0]).max() <= 1e-9 * np.abs(t["dpose"]).max()


# ---------------------------------------------------------------- the C-ABI surface (fails on a tree without the feature: no such symbol)
def test_params_default_and_struct_sizes(pkg):
    b = pkg.binding
    p = b.DoglegParams(); assert b.lib().gs_dogleg_params_default(C.byref(p)) == 0
    assert (p.struct_size, p.max_trials_after_failure, p.initial_delta) == (C.sizeof(b.DoglegParams), 100, 1e4)
    assert C.sizeof(b.DoglegParams) == 16 and C.sizeof(b.DoglegInfo) == 9 * 4 + 4 + 2 * 8 + 2 * 64 * 8 + 2 * 64 * 4
    assert b.lib().gs_dogleg_params_default(None) == -1
    q = b.dogleg_params(max_trials=3, initial_delta=2.5); assert (q.max_trials_after_failure, q.initial_delta) == (3, 2.5)


def test_header_and_exports_agree(pkg):
    b = pkg.binding
    names = b.declared_symbols(debug=False)
    L = b.lib()
    for s in ("gs_optimize_dogleg", "gs_dogleg_params_default", "gs_multiply_hessian"):
        assert s in names and hasattr(L, s)
    assert len(L.gs_optimize_dogleg.argtypes) == 5 and len(L.gs_multiply_hessian.argtypes) == 5
    txt = open(b.HEADER).read()
    for field in ("max_trials_after_failure", "initial_delta", "delta_initial", "delta_final", "n_gn, n_sd, n_dl", "step_kind[64]", "GS_DOGLEG_DL 2"):
        assert field in txt, field
    sec = txt[txt.index("Powell's dogleg ----"):txt.index("robust kernels ----")]
    assert "not pinned against a g2o build" in sec and "NOT DONE" in sec and "reuse of h_gn" in sec and "lambda-damping" in sec and "Slam mirror" in sec


def test_invalid_parameters_and_refusals_on_host_only_handles(pkg):
    b = pkg.binding
    G = pkg.Graph(device=-2)
    G.add_poses([0, 1], [[0, 0, 0], [1, 0, 0]]); G.add_landmarks([0], [[1.0, 1.0]]); G.set_fixed_pose(0)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(initial_delta=0.0), dict(initial_delta=-1.0), dict(initial_delta=nan), dict(initial_delta=inf), dict(max_trials=0), dict(max_trials=-3)):
        with pytest.raises(b.GsError) as e:
            G.optimize_dogleg(3, **bad)
        assert e.value.code == -1, bad                                  # GS_ERR_INVALID, before anything needs a device
    with pytest.raises(b.GsError) as e:
        G.optimize_dogleg(-1)
    assert e.value.code == -1
    assert b.lib().gs_optimize_dogleg(None, 1, None, None, None) == -1
    with pytest.raises(b.GsError) as e:
        G.optimize_dogleg(3)
    assert e.value.code == -4                                           # GS_ERR_NO_DEVICE
    assert b.lib().gs_optimize_dogleg(G.h, 3, None, None, None) == -4    # NULL params: the defaults
    # the Hessian product: null handle / null v / a value that is not finite on a FREE vertex are invalid; on the fixed pose it is not read
    vp = np.zeros((2, 3)); vl = np.zeros((1, 2)); dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    L = b.lib()
    assert L.gs_multiply_hessian(None, dp(vp), dp(vl), None, None) == -1
    assert L.gs_multiply_hessian(G.h, None, dp(vl), None, None) == -1 and L.gs_multiply_hessian(G.h, dp(vp), None, None, None) == -1
    for bad in (nan, inf):
        v = vp.copy(); v[1, 2] = bad
        with pytest.raises(b.GsError) as e:
            G.multiply_hessian(v, vl)
        assert e.value.code == -1
        w = vl.copy(); w[0, 1] = bad
        with pytest.raises(b.GsError) as e:
            G.multiply_hessian(vp, w)
        assert e.value.code == -1
    v = vp.copy(); v[0, 0] = nan
    with pytest.raises(b.GsError) as e:
        G.multiply_hessian(v, vl)
    assert e.value.code == -4                                           # nothing invalid about it: GS_ERR_NO_DEVICE
    with pytest.raises(b.GsError) as e:
        G.multiply_hessian(vp, vl)
    assert e.value.code == -4
    G.dist_configure(0, 2)
    with pytest.raises(b.GsError) as e:
        G.optimize_dogleg(3)
    assert e.value.code == -1 and "shard" in str(e.value)               # a sharded handle: GS_ERR_INVALID
    with pytest.raises(b.GsError) as e:
        G.multiply_hessian(vp, vl)
    assert e.value.code == -1 and "shard" in str(e.value)
    G.close()
