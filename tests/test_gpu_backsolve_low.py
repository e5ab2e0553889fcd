"""GPU tests of the light polling launch of the backward solve (gs_debug_options.bs_low; k_backsolve3<BS_LOW>): the wide levels
below the flagged launch in one launch whose fronts poll their boundary rows.

Its arithmetic and order are the per-level light launch's, so the merged launch on (bs_low = 1), off (bs_low = 0) and one launch per
level (tree = 0) must give the same estimates bit for bit, and each must agree with the oracle to 1e-9 (the bar of
test_solver_launch_modes_give_the_same_answer).  leaf_kernel = 2 forces the leaf launches, without which these sizes have no level
below the flagged launch.  bs_wide = 0 puts every level but the root into the polling launch: a chain as deep as the tree."""
import numpy as np
import pytest

from conftest import make_oracle_graph, random_graph

pytestmark = pytest.mark.gpu


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def fresh(pkg, arrays, **debug):
    g = pkg.Graph(debug=dict(leaf_kernel=2, **debug)); g.load_bench_graph(arrays)
    return g


_ref = {}


@pytest.fixture(scope="module")
def reference(pkg, po, bench_graphs):
    """per graph size, computed once: the oracle's estimates after 4 iterations and the solver's with one launch per level"""
    def get(N, M):
        if (N, M) not in _ref:
            _, g = bench_graphs(N, M)
            og = make_oracle_graph(po, g); og.optimize(4, ordering=1)
            G = fresh(pkg, g, tree=0); done, st = G.optimize(4)
            assert done == 4 and st.numeric_failure == 0
            _ref[(N, M)] = (g, og.poses().copy(), og.landmarks().copy(), G.poses().copy(), G.landmarks().copy()); G.close()
        return _ref[(N, M)]
    return get


def n_backsolve_launches(G):
    return sum(1 for r in G.debug_schedule()["launches_tree"] if int(r[0]) in (6, 7, 8))


@pytest.mark.parametrize("env", [dict(), dict(bs_wide=0), dict(bs_wide=8), dict(tickets=1), dict(block_fronts=0), dict(bs_wide=0, tickets=1)],
                         ids=lambda e: "-".join("%s%d" % kv for kv in e.items()) or "default")
@pytest.mark.parametrize("N,M", [(1000, 200), (10000, 2000)])
def test_merged_launch_on_off_and_per_level_agree_bit_for_bit(pkg, reference, N, M, env):
    g, P_o, L_o, P_lvl, L_lvl = reference(N, M)
    outs = []
    for low in (1, 0):
        G = fresh(pkg, g, bs_low=low, **env); done, st = G.optimize(4)
        assert done == 4 and st.numeric_failure == 0 and st.fell_back == 0, (env, low)
        nb = n_backsolve_launches(G)
        assert (nb == 2) if low else (nb >= 2), (env, low, nb)         # the merged launch really ran: one launch behind the flagged one
        outs.append((G.poses().copy(), G.landmarks().copy())); G.close()
    for P, L in outs:
        assert rel(P, P_o) < 1e-9 and rel(L, L_o) < 1e-9, env
        assert np.array_equal(P, P_lvl) and np.array_equal(L, L_lvl), env
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("seed,shape", [(105, dict(n_poses=150, n_lms=12, obs_per_pose=3, extra_pp=25)), (103, dict(n_poses=40, n_lms=25))])
def test_irregular_trees_one_step(pkg, po, seed, shape):
    """Two graphs of test_irregular_graphs_one_step_matches_oracle whose fronts all fit a wave (61 scalars at most: with a bigger front the
    launches are table-driven and the merged launch does not run).  Seed 105: 45 fronts on 5 levels, four leaves that hang under fronts
    above level 1 (their boundary rows belong to grandparents and beyond), a front with five children; seed 103: 13 fronts, one with
    four children.  Every level but the root polls (bs_wide = 0)."""
    g = random_graph(seed, **shape)
    og = make_oracle_graph(po, g); og.build_system(); og.apply_update(og.solve_ldlt(0)); dp_o, dl_o = og.delta()
    scale = max(np.abs(dp_o).max(), np.abs(dl_o).max())
    outs = []
    for env in (dict(bs_low=1), dict(bs_low=0), dict(tree=0)):
        G = fresh(pkg, g, bs_wide=0, **env); done, st = G.optimize(1); dp, dl = G.export_delta()
        assert done == 1 and st.numeric_failure == 0 and st.fell_back == 0, env
        assert st.max_front <= 63
        if "bs_low" in env:
            assert n_backsolve_launches(G) == (2 if env["bs_low"] else G.debug_schedule()["bs_l0"] + 1)
        assert np.abs(dp - dp_o).max() / scale < 1e-9 and np.abs(dl - dl_o).max() / scale < 1e-9, (env, st.max_front)
        outs.append((dp.copy(), dl.copy())); G.close()
    for dp, dl in outs[1:]:
        assert np.array_equal(dp, outs[0][0]) and np.array_equal(dl, outs[0][1])


def test_one_handle_follows_the_option_between_calls(pkg, po, bench_graphs):
    """the option is a plan field: toggled between two calls of one handle, the second call runs the other launches (no stale
    schedule).  Two handles toggle in opposite directions: the same two calls, the same estimates bit for bit."""
    _, g = bench_graphs(1000, 200)
    og = make_oracle_graph(po, g); og.optimize(2, ordering=1); og.optimize(2, ordering=1)
    outs = []
    for first in (1, 0):
        G = fresh(pkg, g, bs_low=first, bs_wide=0)
        for low in (first, 1 - first):
            G.set_debug(bs_low=low)
            done, st = G.optimize(2)
            assert done == 2 and st.numeric_failure == 0 and st.fell_back == 0
            S = G.debug_schedule()
            assert S["bs_l0"] > 1 and G.debug_options().bs_low == low
            assert n_backsolve_launches(G) == (2 if low else S["bs_l0"] + 1), (first, low)
        outs.append((G.poses().copy(), G.landmarks().copy())); G.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert rel(outs[0][0], og.poses()) < 1e-9 and rel(outs[0][1], og.landmarks()) < 1e-9
