"""gs_multiply_hessian (the device Hessian-vector product, csrc/gs_hmul.hip) entry by entry.

1. Against the GPU's own exported blocks: after gs_linearize, G.multiply_hessian(v) is compared with hmul_ref.multiply on
   G.export_system() — the exported blocks are existing, separately tested code (test_gpu_lin_exact.py, test_gpu_side_exact.py), so only
   the product is under test.  Cases: every case of lin_shapes.CASES at its forced lane count and every case of side_shapes.CASES on each
   of its paths (70 to 300-pose graphs: the hub pose, duplicate edges, a fixed pose and a fixed landmark, a pose without observations, a
   partial last wave tile, priors, polar edges, an inactive edge, robust weights, launch255 / launch257).  Vectors: a random v, v = b of
   the export, unit vectors on the hub pose, on the landmark three wave tiles see, and on a fixed vertex.  Bound per component i:
   2 (n_i + 2) 2^-53 (|H| |v|)_i with n_i the products of row i (hmul_ref.py derives it); rows of fixed vertices exactly 0; symmetry
   u^T (H v) - v^T (H u) within the same bound summed over the components.
2. A grown plan (tail poses and tail cones): against hmul_ref on the grown handle's own export, the rounding bound alone; and, as a
   second line, on the oracle's linearize_blocks() at the same estimates with 1e-11 max_i (|H| |v|)_i added — the project's own H-block
   bound (test_gpu_parity.py); plain and with Huber.
3. The damping of a preceding gs_optimize_lm trial is in the product.
4. The call changes no state.
Every test prints its worst err / bound before it asserts (-s); the printed run is profiles/hmul_gpu_suite.txt.

Measured on an MI355X: worst err / bound over all 98 cases of part 1 0.142 (t1_groups, cauchy, priors_groups), fused and gather alike; the
symmetry defect 2 to 4 orders under its bound; on the grown plan against its own export 0.101 (0.097 with Huber), and against the oracle's
blocks the rounding part is invisible beside the 1e-11 block term (worst err / bound 0.000 to three digits); the damping difference at most 0.03 of its tolerance."""
import numpy as np
import pytest

import hmul_ref as hr
import lin_shapes as ls
import robust_ref as rr
import side_shapes as ss
from conftest import make_oracle_graph
from test_gpu_lm import GROWN_H, free_masks, fresh, grown

pytestmark = pytest.mark.gpu


def vectors(g, B, notes, seed=0):
    """[(label, v_pose, v_lm, zero)]: random, b, unit vectors on the hub pose / the wide landmark / a fixed pose and a fixed landmark;
    zero: the whole product must be zero (True), must not be (False), no claim (None)"""
    N, M = len(B["Hpp_diag"]), len(B["Hll_diag"])
    rng = np.random.default_rng(seed)
    out = [("random", rng.normal(size=(N, 3)) * [1, 1, 0.2], rng.normal(size=(M, 2)), None), ("b", B["b_pose"].copy(), B["b_lm"].copy(), None)]
    def unit(kind, i, c, zero):
        vp, vl = np.zeros((N, 3)), np.zeros((M, 2)); (vp if kind == "pose" else vl)[i, c] = 1.0
        return ("unit %s %d.%d" % (kind, i, c), vp, vl, zero)
    out += [unit("pose", notes["hub"], 2, False), unit("pose", notes["hub"], 0, False), unit("landmark", notes["wide"], 1, False)]
    out += [unit("pose", int(g["fixed_poses"][0]), 1, True), unit("landmark", int(g["fixed_landmarks"][0]), 0, True)]
    return out


def hold(G, g, B, notes, tag, extra_rel=0.0):
    """every vector of vectors() against hmul_ref on the blocks B; symmetry with two random vectors; returns the worst err / bound"""
    worst = 0.0; prods = {}
    for label, vp, vl, zero in vectors(g, B, notes):
        yp, yl = G.multiply_hessian(vp, vl)
        _, _, Sp, Sl, _, _ = hr.multiply(B, g, vp, vl)
        extra = extra_rel * max(Sp.max(initial=0.0), Sl.max(initial=0.0))
        worst = max(worst, hr.check(yp, yl, B, g, vp, vl, extra=extra))
        if zero is not None:                                             # a fixed vertex's column is zero, a free one's is not
            assert (not yp.any() and not yl.any()) if zero else (yp.any() or yl.any()), label
        prods[label] = (vp, vl, yp, yl)
    # symmetry: u = random, v = b
    (up, ul, Hup, Hul), (vp, vl, Hvp, Hvl) = prods["random"], prods["b"]
    fp, fl = hr.masks(g, len(up), len(ul)); ld = np.longdouble
    z = lambda a, m: np.where(m[:, None], a, 0.0).astype(ld)
    lhs = (z(up, fp) * Hvp).sum() + (z(ul, fl) * Hvl).sum(); rhs = (z(vp, fp) * Hup).sum() + (z(vl, fl) * Hul).sum()
    bnd = 0.0
    for a_p, a_l, b_p, b_l in ((up, ul, vp, vl), (vp, vl, up, ul)):                 # |a|^T bound(H b)
        _, _, Sp, Sl, n_p, n_l = hr.multiply(B, g, b_p, b_l); bp, bl = hr.bound(Sp, Sl, n_p, n_l)
        ex = extra_rel * max(Sp.max(initial=0.0), Sl.max(initial=0.0))
        bnd += float((np.abs(z(a_p, fp)) * (bp + ex)).sum() + (np.abs(z(a_l, fl)) * (bl + ex)).sum())
    sym = float(abs(lhs - rhs))
    print("%-28s worst err / bound %.3f | symmetry |u.Hv - v.Hu| %.3e, bound %.3e" % (tag, worst, sym, bnd))
    assert sym <= bnd
    return worst


# ---------------------------------------------------------------- 1. against the exported blocks
@pytest.mark.parametrize("name", list(ls.CASES))
def test_product_entry_by_entry_linearisation_shapes(pkg, name):
    g, _, notes = ls.graph(name)
    G = pkg.Graph(device=0, **ls.handle_kw(name)); G.load_bench_graph(g)
    G.initialize_optimization(); G.linearize()
    hold(G, g, G.export_system(), notes, name)
    G.close()


@pytest.mark.parametrize("name,path", ss.RUNS)
def test_product_entry_by_entry_side_passes(pkg, name, path):
    c = ss.case(name)
    G = ss.load(pkg.Graph(device=0, **ss.handle_kw(name, path)), name)
    G.initialize_optimization(); G.linearize()
    hold(G, c["g"], G.export_system(), c["notes"], "%s %s" % (name, "gather" if path == "gather" else "T=%d" % path))
    G.close()


def test_refusals_on_the_device(pkg, bench_graphs):
    """nothing linearised yet — no plan on the device, a plan that has not linearised, a growth step since the last linearisation —:
    GS_ERR_NOT_INITIALIZED; a value that is not finite on a free vertex: GS_ERR_INVALID, on a fixed one: ignored"""
    _, g = bench_graphs(50, 30)
    G = fresh(pkg, g); N, M = len(g["pose_est"]), len(g["lm_est"])
    for step in (lambda: None, G.initialize_optimization):
        step()
        with pytest.raises(pkg.binding.GsError) as e:
            G.multiply_hessian(np.zeros((N, 3)), np.zeros((M, 2)))
        assert e.value.code == -6
    H, full = grown(pkg, bench_graphs(1000, 200)[1])                 # (its last act is the growth step)
    v = (np.zeros((len(full["pose_est"]), 3)), np.zeros((len(full["lm_est"]), 2)))
    with pytest.raises(pkg.binding.GsError) as e:
        H.multiply_hessian(*v)
    assert e.value.code == -6
    H.linearize(); H.multiply_hessian(*v); H.close()
    G.linearize()
    fp, fl = free_masks(g)
    v = np.ones((N, 3)); v[np.flatnonzero(fp)[0], 1] = np.inf
    with pytest.raises(pkg.binding.GsError) as e:
        G.multiply_hessian(v, np.zeros((M, 2)))
    assert e.value.code == -1
    v = np.ones((N, 3)); w = np.ones((M, 2)); y0 = G.multiply_hessian(v, w)
    v[~fp] = np.nan; w[~fl] = np.inf; y1 = G.multiply_hessian(v, w)
    assert (~fp).any() and np.array_equal(y0[0], y1[0]) and np.array_equal(y0[1], y1[1])
    G.close()


# ---------------------------------------------------------------- 2. a grown plan
@pytest.mark.parametrize("huber", [0, 1])
def test_product_on_a_grown_plan(pkg, po, bench_graphs, huber):
    """tail poses and tail cones (grown() asserts both): the tail arenas, the tail's edge tables and the old vertices' diagonal shares of
    tail edges (read where the fronts read them: Hpp_diag, the first partial-sum slot) against the grown handle's OWN exported blocks
    (test_gpu_tail_exact.py holds those to the exact reference) within the rounding bound alone; unit vectors on a tail pose and on a tail
    cone.  Second, looser line: the oracle's blocks at the same estimates with the 1e-11 block term (with Huber: the re-weighted oracle)."""
    G, full = grown(pkg, bench_graphs(1000, 200)[1])
    kernels = {}
    if huber:
        kernels = {"observation": ("huber", rr.median_deltas(full, full["pose_est"], full["lm_est"])[1])}
        G.set_robust_kernel("observation", *kernels["observation"])
    G.linearize()
    B = make_oracle_graph(po, rr.reweighted(full, full["pose_est"], full["lm_est"], kernels) if huber else full).linearize_blocks()
    N, M = len(full["pose_est"]), len(full["lm_est"])
    notes = dict(hub=N - 1, wide=M - 1)                               # the unit vectors of hold(): the last tail pose, the last tail cone
    st = G.stats(); assert st.n_growths > 0
    worst = hold(G, full, G.export_system(), notes, "grown%s" % (" huber" if huber else ""))
    hold(G, full, B, notes, "grown%s against the oracle" % (" huber" if huber else ""), extra_rel=1e-11)
    # the first tail pose alone: the old pose before it and every cone it sees, old ones included, get their rows through tail edges
    t0 = N - GROWN_H
    vp, vl = np.zeros((N, 3)), np.zeros((M, 2)); vp[t0, 2] = 1.0
    yp, yl = G.multiply_hessian(vp, vl)
    cones = np.unique(full["pl_l"][full["pl_p"] == t0]); free_l = free_masks(full)[1]
    assert yp[t0 - 1].any() and len(cones) > 0 and all(yl[l].any() for l in cones if free_l[l]) and cones.min() < M - 2
    assert worst <= 1.0
    G.close()


# ---------------------------------------------------------------- 3. damping
@pytest.mark.parametrize("gather", [0, 1])
def test_the_lambda_of_a_preceding_lm_trial_is_in_the_product(pkg, bench_graphs, gather):
    """After optimize_lm(1, initial_lambda = lam, max_trials = 1) the system in HBM is that trial's as it was factorised: H at the start
    with lam on every free diagonal scalar.  The product differs from the undamped one by lam v on the free scalars, within the two
    products' rounding bounds plus the rounding of H_jj + lam (2^-52 (|H_jj| + lam) |v_j|)."""
    _, g = bench_graphs(1000, 200)
    G = fresh(pkg, g, linearize_gather=gather)
    G.initialize_optimization(); G.linearize()
    B = G.export_system(); N, M = len(g["pose_est"]), len(g["lm_est"])
    rng = np.random.default_rng(3); vp, vl = rng.normal(size=(N, 3)), rng.normal(size=(M, 2))
    y0p, y0l = G.multiply_hessian(vp, vl)
    lam = 0.01 * max(np.abs(B["Hpp_diag"]).max(), np.abs(B["Hll_diag"]).max())
    done, st, info = G.optimize_lm(1, initial_lambda=lam, max_trials=1)
    assert info["trials"] == 1 and info["lambda_initial"] == lam
    y1p, y1l = G.multiply_hessian(vp, vl)
    fp, fl = free_masks(g)
    _, _, Sp, Sl, n_p, n_l = hr.multiply(B, g, vp, vl); bp, bl = hr.bound(Sp + lam * np.abs(vp), Sl + lam * np.abs(vl), n_p + 1, n_l + 1)
    dp = y1p - y0p - lam * np.where(fp[:, None], vp, 0.0); dl = y1l - y0l - lam * np.where(fl[:, None], vl, 0.0)
    tp = 2 * bp + 4 * hr.U * (np.abs(B["Hpp_diag"][:, (0, 4, 8)]) + lam) * np.abs(vp); tl = 2 * bl + 4 * hr.U * (np.abs(B["Hll_diag"][:, (0, 3)]) + lam) * np.abs(vl)
    print("gather=%d lambda %.4g: worst |y1 - y0 - lam v| / tolerance: poses %.3f landmarks %.3f; |lam v| max %.3g" % (
        gather, lam, (np.abs(dp)[fp] / tp[fp]).max(), (np.abs(dl)[fl] / tl[fl]).max(), lam * np.abs(vp).max()))
    assert np.all(np.abs(dp) <= tp) and np.all(np.abs(dl) <= tl)
    assert not y1p[~fp].any() and not y1l[~fl].any()
    G.close()


# ---------------------------------------------------------------- 4. no state
def test_the_product_changes_no_state(pkg, bench_graphs):
    """estimates, chi2, export_system() and a following optimize(1) are bit-identical with and without a multiply_hessian call between"""
    _, g = bench_graphs(1000, 200)
    N, M = len(g["pose_est"]), len(g["lm_est"]); v = (np.ones((N, 3)), np.ones((M, 2)))
    out = []
    for call in (False, True):
        G = fresh(pkg, g); G.initialize_optimization(); G.linearize()
        if call:
            G.multiply_hessian(*v)
        S = G.export_system(); chi = G.chi2(); P, L = G.poses(), G.landmarks()
        if call:
            G.multiply_hessian(*v)
        done, st = G.optimize(1)
        if call:
            G.multiply_hessian(*v)
        out.append((S, chi, P, L, done, st.chi2_initial, st.chi2_final, G.poses(), G.landmarks(), G.export_delta()))
        G.close()
    a, b = out
    assert all(np.array_equal(a[0][k], b[0][k]) for k in a[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert a[4:7] == b[4:7] and np.array_equal(a[7], b[7]) and np.array_equal(a[8], b[8])
    assert np.array_equal(a[9][0], b[9][0]) and np.array_equal(a[9][1], b[9][1])
