"""GPU tests of the linearisation pass, entry by entry, at every lane count of k_linearize_ell<T> and on the gather kernels.

Every case of tests/lin_shapes.py (the census in test_lin_exact_cpu.py proves which path each one reaches) is linearised on a handle with
the forced gs_debug_options.ell_lanes, and every entry of the six arrays of gs_export_system, gs_chi2 and the per-edge s of
gs_get_edge_chi2 are held to
        |got - exact| <= C(n) u S,      C(n) = 2 (34 + n), with a robust kernel 2 (71 + n),      u = 2^-53
against the mpmath linearisation of tests/lin_exact_ref.py (S: the entry's magnitude with every elementary product by absolute value,
n: the edges summed into it; the count behind C is in that module's docstring).  A reference with one term off by 1e-9 must fail the
same bound (lin_exact_ref.check_can_fail / assert_two_sided).  Every case that the fused kernel takes runs again with
linearize_gather = 1; an iteration of gs_optimize is held to the same bound before and after its update.

Measured worst err / (u S) per case and array: NOT YET RECORDED — this module has not run on an MI355X (the CPU oracle's figures on the same
cases, 2.4 .. 5.4, are in test_lin_exact_cpu.py); the run prints one line per case for this table.
"""
import numpy as np
import pytest

import lin_exact_ref as lx
import lin_shapes as ls
from plan_exec import Plan

pytestmark = pytest.mark.gpu
_exact = {}


def exact(name):
    """the reference of a case at its own estimates: computed once, shared by the fused, the gather and the iteration tests"""
    if name not in _exact:
        g, kernels, _ = ls.graph(name)
        _exact[name] = lx.linearize(g, kernels)
    return _exact[name]


def fresh(pkg, name, gather=False):
    g, _, _ = ls.graph(name)
    G = pkg.Graph(device=0, **ls.handle_kw(name, gather)); G.load_bench_graph(g)
    return G, g


def hold(G, X, name, tag, with_chi2=True):
    """the handle's last linearisation, its chi2 and its per-edge s against the reference X, both ways"""
    blocks = G.export_system()
    chi2 = G.chi2() if with_chi2 else None
    s_pp = G.edge_chi2("odometry")[0] if with_chi2 else None; s_pl = G.edge_chi2("observation")[0] if with_chi2 else None
    worst = lx.check(X, blocks, chi2, s_pp, s_pl, tag=tag)
    moved = lx.check_can_fail(X, blocks, chi2, tag=tag)
    c = ls.CASES[name]
    lx.assert_two_sided(moved, far=bool(c.get("far")), robust=bool(c.get("robust")), tag=tag)
    print("%-28s err / (u S): %s | perturbed: %s" % (tag, " ".join("%s %.2f" % kv for kv in worst.items()),
          " ".join("%s %s" % (k, "-" if v is None else "%.3g%s" % (v[1], "*" if v[3] else "")) for k, v in moved.items())))
    return worst


@pytest.mark.parametrize("name", list(ls.CASES))
def test_linearize_entry_by_entry(pkg, name):
    c = ls.CASES[name]
    G, g = fresh(pkg, name)
    G.initialize_optimization(); G.linearize()
    P = Plan(G.plan_export())
    assert (P.ell_T, P.ell_R) == (c["T"] or 8, c["R"])
    assert (P.ell_R > ls.LIN_R) == c["fallback"]                   # more slots than the fused kernel has: the plan says the gather kernels ran
    hold(G, exact(name), name, name + (" (gather: R = %d)" % P.ell_R if c["fallback"] else ""))
    G.close()


@pytest.mark.parametrize("name", [n for n, c in ls.CASES.items() if not c["fallback"]])
def test_gather_kernels_entry_by_entry(pkg, name):
    G, g = fresh(pkg, name, gather=True)
    G.initialize_optimization(); G.linearize()
    hold(G, exact(name), name, name + " gather")
    G.close()


@pytest.mark.parametrize("name", ["t1_r4", "t2_k8", "t4_k16"])
def test_an_iteration_runs_the_fused_pass_before_and_after_its_update(pkg, name):
    """gs_optimize(1): the exported system is that iteration's (test_the_export_holds_the_last_linearisation) and meets the bound at the
    estimates before the update; gs_linearize afterwards meets it at the new ones — with the cos / sin k_update refreshed, at this T"""
    G, g = fresh(pkg, name)
    done, st = G.optimize(1)
    assert done == 1 and st.numeric_failure == 0
    hold(G, exact(name), name, name + " iteration", with_chi2=False)
    poses, lms = G.poses(), G.landmarks()
    assert np.abs(poses - g["pose_est"]).max() > 1e-3
    G.linearize()
    hold(G, lx.linearize(g, None, poses, lms), name, name + " after update")
    G.close()
