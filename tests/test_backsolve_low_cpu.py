"""CPU tests of the light polling launch of the backward solve (gs_debug_options.bs_low; csrc/gs_schedule.hpp, walk_backsolve_levels)
through gs_debug_schedule_export on host-only handles, in the pattern of test_schedule_cpu.py.

In whole-tree mode the levels below the flagged launch (bs_l0 - 1 .. 0) share ONE launch whose fronts poll their boundary rows; it is
recorded with the flagged kind.  Asserted: the backward-solve launches still cover every level position exactly once, at most one
launch follows the flagged one, the launch walks its positions from the top down so that a parent always comes before its child, and
its LDS fits a workgroup.  The per-level record (the mode of a handle after a flag timeout) does not know the option.  No HIP code runs."""
import numpy as np
import pytest

from plan_exec import Plan

LDS_MAX = 160 * 1024
K_BTREE, K_BLEVEL, K_BTAB = 6, 7, 8
PLANS = [(240, 200), (1000, 200)]
WIDE = [0, 8, 2048]
_cache = {}


@pytest.fixture(scope="module")
def sched(pkg, bench_graphs):
    def get(n, m, bs_wide, bs_low):
        key = (n, m, bs_wide, bs_low)
        if key not in _cache:
            G = pkg.Graph(device=-2, debug=dict(leaf_min=0, bs_wide=bs_wide, bs_low=bs_low)); G.load_bench_graph(bench_graphs(n, m)[1])
            G.plan_build_host()
            _cache[key] = (G.debug_schedule(), Plan(G.plan_export())); G.close()
        return _cache[key]
    return get


def backsolve(S, mode):
    return [tuple(int(v) for v in r) for r in S[mode] if int(r[0]) in (K_BTREE, K_BLEVEL, K_BTAB)]


def test_the_option_defaults_to_the_merged_launch(pkg):
    d = pkg.binding.DebugOptions(); assert pkg.binding.lib().gs_debug_options_default(d) == 0
    assert d.bs_low == 1 and d.bs_wide in (512, 1024, 2048)


@pytest.mark.parametrize("bs_wide", WIDE)
@pytest.mark.parametrize("n,m", PLANS)
def test_one_launch_behind_the_flagged_one_covers_the_wide_levels_top_down(sched, n, m, bs_wide):
    S, P = sched(n, m, bs_wide, 1)
    n_own, os_ = S["n_own"], S["own_start"]
    assert S["n_shared"] == 0 and S["tables"] == 0 and S["leaf_n"] == os_[1] > 0 and S["bs_l0"] >= 1
    recs = backsolve(S, "launches_tree")
    # every level position exactly once
    seen = np.zeros(n_own, dtype=np.int64)
    for kind, first, count, lds, cls, table in recs:
        assert table < 0 and count > 0 and 0 <= first and first + count <= n_own and 0 <= lds <= LDS_MAX
        seen[first:first + count] += 1
    assert (seen == 1).all()
    # the flagged launch over levels >= bs_l0, then at most one launch: the merged one over everything below, flagged kind
    l0 = S["bs_l0"]
    assert recs[0][:3] == (K_BTREE, int(os_[l0]), n_own - int(os_[l0]))
    assert len(recs) == 2, recs
    kind, first, count, lds, cls, table = recs[1]
    assert (kind, first, count) == (K_BTREE, 0, int(os_[l0]))
    assert 0 < lds <= LDS_MAX                                            # (its LDS is the schedule's: recorded, unlike the flagged launch's)
    if bs_wide == 0:                                                     # every level but the root: a polling chain as deep as the tree
        assert l0 == S["n_levels"] - 1 and S["n_levels"] > 2
    if bs_wide == 2048:                                                  # no level of these plans is that wide: the leaves alone
        assert l0 == 1
    # the launch takes its positions downwards: a parent inside it sits at a higher position than its child, i.e. comes first;
    # a parent outside it ran in the flagged launch before
    front_at = S["own_fronts"]; pos_of = np.full(P.n_fronts, -1); pos_of[front_at] = np.arange(n_own)
    n_inside = 0
    for q in range(first, first + count):
        pa = int(P.parent[front_at[q]])
        if pa < 0:
            continue
        pq = int(pos_of[pa])
        assert pq > q, (q, pq)
        if pq < first + count:
            n_inside += 1
            assert P.level[pa] > P.level[front_at[q]]
        else:
            assert P.level[pa] >= l0
    assert (n_inside > 0) == (l0 > 1)


@pytest.mark.parametrize("bs_wide", WIDE)
@pytest.mark.parametrize("n,m", PLANS)
def test_the_switch_restores_a_launch_per_level_and_the_per_level_mode_ignores_it(sched, n, m, bs_wide):
    (S1, _), (S0, _) = sched(n, m, bs_wide, 1), sched(n, m, bs_wide, 0)
    os_ = S0["own_start"]; l0 = S0["bs_l0"]
    assert S1["bs_l0"] == l0
    # switch off: the flagged launch, then levels l0 - 1 .. 0 a launch each
    want = [(K_BTREE, int(os_[l0]), S0["n_own"] - int(os_[l0]))] + [(K_BLEVEL, int(os_[l]), int(os_[l + 1] - os_[l])) for l in range(l0 - 1, -1, -1)]
    assert [r[:3] for r in backsolve(S0, "launches_tree")] == want
    # everything but the backward-solve launches of whole-tree mode is the same record
    assert np.array_equal(S1["launches_level"], S0["launches_level"])
    fac = lambda S: [tuple(int(v) for v in r) for r in S["launches_tree"] if int(r[0]) not in (K_BTREE, K_BLEVEL, K_BTAB)]
    assert fac(S1) == fac(S0)
    for k in ("leaf_n", "leaf_slot", "n_subtrees", "block_n", "own_start", "own_fronts"):
        assert np.array_equal(S1[k], S0[k])


def test_plans_without_a_leaf_launch_have_no_merged_launch(pkg, bench_graphs):
    """few leaves (<= leaf_min): level 0 is in the flagged launch already, bs_l0 = 0, nothing to merge"""
    G = pkg.Graph(device=-2, debug=dict(bs_low=1)); G.load_bench_graph(bench_graphs(240, 200)[1]); G.plan_build_host()
    S = G.debug_schedule(); G.close()
    assert S["bs_l0"] == 0 and [r[0] for r in backsolve(S, "launches_tree")] == [K_BTREE]
