"""CPU tests of the launch schedule (csrc/gs_schedule.cpp) through gs_debug_schedule_export on host-only handles.

The schedule — which solver launches an iteration is made of — is a function of the plan and the options, built with the plan.  The
export walks it with the same traversal the enqueue path launches from, once for whole-tree mode and once for one launch per level
(the mode of a handle after a flag timeout).  Asserted here, for every plan and both modes: the launches cover every level position
exactly once per phase, respect the elimination tree's order, stay within the LDS of a workgroup, and the record has no history.
No HIP code runs here."""
import numpy as np
import pytest

from plan_exec import Plan

LDS_MAX = 160 * 1024
FACTOR_TABLES, BACKSOLVE_TABLES = (0, 2, 3), (1, 4)
K_TREE, K_LEAF, K_LEVEL, K_TOP, K_FTAB, K_BTREE, K_BLEVEL, K_BTAB = 1, 2, 3, 4, 5, 6, 7, 8

# name -> (graph, debug options, sharded, max_front the host plan reports (None: not pinned))
#   big-smallest: the smallest track.generate(n, m, 16) graph there is (3 poses; 16 in view need 48 cones): ONE front of 95 scalars, kind 2
#   big: 100 poses / 50 cones, 16 in view: max_front 98, fronts of 64-79 (kind 4) and 80-111 (kind 2); no plan of this generator
#        holds a front over 111 with default options (looked for up to 2000 poses) ...
#   big-wide: ... so the third kind (112-159, kind 3) comes from the same graph with leaf_poses = 24: max_front 134, kinds 2 and 3
CASES = {
    "lap": ((240, 200, None), {}, False, None),
    "lap-leaf0": ((240, 200, None), dict(leaf_min=0), False, None),
    "bench1000": ((1000, 200, None), {}, False, None),
    "bench1000-leaf0": ((1000, 200, None), dict(leaf_min=0), False, None),
    "big-smallest": ((3, 48, 16), {}, False, 95),
    "big": ((100, 50, 16), {}, False, 98),
    "big-wide": ((100, 50, 16), dict(leaf_poses=24), False, 134),
    "bench1000-shared": ((1000, 200, None), dict(force_shared_top=3), True, None),
    "big-shared": ((100, 50, 16), dict(force_shared_top=3), True, 98),
}
_cache = {}


def handle(pkg, bench_graphs, frontend, name):
    (n, m, k), debug, shared, _ = CASES[name]
    g = bench_graphs(n, m)[1] if k is None else pkg.track.bench_graph(pkg.track.generate(n, m, k), frontend)
    G = pkg.Graph(device=-2, debug=dict(debug)); G.load_bench_graph(g)
    if shared:
        G.dist_configure(0, 1)
    G.plan_build_host()
    return G


@pytest.fixture(scope="module")
def case(pkg, bench_graphs, frontend):
    def get(name):
        if name not in _cache:
            G = handle(pkg, bench_graphs, frontend, name)
            _cache[name] = (G.debug_schedule(), Plan(G.plan_export())); G.close()
        return _cache[name]
    return get


def covered(S, rec):
    """level positions of one launch, in table-entry order where a table drives it"""
    kind, first, count, lds, cls, table = (int(v) for v in rec)
    if table < 0:
        return [(p, 0) for p in range(first, first + count)]
    out = []
    for e, (pos, kc) in enumerate(S["tab"][table][first:first + count]):
        k, c = int(kc) & 255, int(kc) >> 8
        if k == 0:
            out += [(p, e) for p in (range(pos, pos + c) if table in FACTOR_TABLES else range(pos, pos - c, -1))]
        else:
            out.append((int(pos), e))
    return out


def level_of(S, pos):
    if pos < S["n_own"]:
        return int(np.searchsorted(S["own_start"], pos, side="right")) - 1
    return int(np.searchsorted(S["shared_start"], pos - S["shared_base"], side="right")) - 1


@pytest.mark.parametrize("mode", ["launches_tree", "launches_level"])
@pytest.mark.parametrize("name", list(CASES))
def test_launches_cover_every_position_once_in_tree_order(case, name, mode):
    S, P = case(name)
    n_own, n_sh, base = S["n_own"], S["n_shared"], S["shared_base"]
    assert base == n_own and n_own + n_sh == P.n_fronts
    front_at = np.concatenate([S["own_fronts"], S["shared_fronts"]])
    pos_of = np.full(P.n_fronts, -1); pos_of[front_at] = np.arange(len(front_at))
    assert sorted(front_at.tolist()) == list(range(P.n_fronts))
    # phases: own factor + top (the dependent ones), contributions (independent of each other by construction: excluded from the
    # order checks), backward solve
    where = {"factor": {}, "contrib": {}, "backsolve": {}}
    per_launch = []
    for li, rec in enumerate(S[mode]):
        kind, first, count, lds, cls, table = (int(v) for v in rec)
        assert 0 <= lds <= LDS_MAX, (name, rec)
        assert count > 0
        if kind in (K_BTREE, K_BLEVEL, K_BTAB):
            phase = "backsolve"
        elif (kind == K_LEVEL and cls == 1) or (kind == K_FTAB and table == 2):
            phase = "contrib"
        else:
            phase = "factor"
        if table >= 0:
            assert table in (FACTOR_TABLES if phase != "backsolve" else BACKSOLVE_TABLES)
            assert 0 <= first and first + count <= len(S["tab"][table])
        cov = covered(S, rec)
        per_launch.append((phase, [p for p, _ in cov]))
        for p, e in cov:
            assert 0 <= p < n_own + n_sh
            assert p not in where[phase], "%s: position %d covered twice in phase %s" % (name, p, phase)
            where[phase][p] = (li, e, table)
    assert sorted(where["factor"]) == list(range(n_own + n_sh))          # every own position once, every shared one once (the top)
    assert sorted(where["backsolve"]) == list(range(n_own + n_sh))
    assert sorted(where["contrib"]) == list(range(base, base + n_sh))
    # order: a child never after its parent in the factor phase, never before it in the backward solve.  Inside a launch that is
    # not table-driven the kernel orders its fronts by their flags; in per-level mode no launch may hold a front AND its child
    tree = mode == "launches_tree"
    for s in range(P.n_fronts):
        p = int(P.parent[s])
        if p < 0:
            continue
        c, q = int(pos_of[s]), int(pos_of[p])
        (lc, ec, tc), (lp, ep, _) = where["factor"][c], where["factor"][q]
        assert (lc, ec) < (lp, ep) or (tree and lc == lp and tc < 0), (name, mode, "factor", s, p)
        (lc, ec, tc), (lp, ep, _) = where["backsolve"][c], where["backsolve"][q]
        assert (lp, ep) < (lc, ec) or (tree and lc == lp and tc < 0), (name, mode, "backsolve", s, p)
        if not tree:
            assert where["factor"][c][0] != where["factor"][q][0] and where["backsolve"][c][0] != where["backsolve"][q][0]
    if not tree:
        for phase, ps in per_launch:
            if phase != "contrib":
                fr = set(int(front_at[p]) for p in ps)
                assert not any(int(P.parent[s]) in fr for s in fr), (name, "a per-level launch holds a front and its child")


@pytest.mark.parametrize("name", list(CASES))
def test_tables_and_scalar_decisions(case, name):
    S, P = case(name)
    want_mf = CASES[name][3]
    if want_mf is not None:
        assert P.max_front == want_mf
    f = P.npiv + P.nbnd
    assert S["factor_variant"] == 3 and S["tables"] == (1 if P.max_front > 63 else 0)
    front_at = np.concatenate([S["own_fronts"], S["shared_fronts"]])
    kinds = set()
    for t, tab in enumerate(S["tab"]):
        if not S["tables"]:
            assert len(tab) == 0
            continue
        n_fronts = 0
        for pos, kc in tab:
            k, c = int(kc) & 255, int(kc) >> 8
            kinds.add(k)
            if k == 0:                                           # a wave each, at most four, never across a level
                assert 1 <= c <= 4
                ps = range(pos, pos + c) if t in FACTOR_TABLES else range(pos, pos - c, -1)
                assert len({level_of(S, p) for p in ps}) == 1
                assert all(f[front_at[p]] <= 63 for p in ps)
                n_fronts += c
            else:
                size = int(f[front_at[pos]])
                assert (k == 1 and size <= 63) or (k == 4 and 64 <= size <= 79) or (k == 2 and 80 <= size <= 111) or (k == 3 and 112 <= size <= 159)
                n_fronts += 1
        # the entries' counts sum to the fronts the table covers: the own lists everything above the leaf launch, the shared ones everything
        assert n_fronts == {0: S["n_own"] - S["leaf_n"], 1: S["n_own"]}.get(t, S["n_shared"])
    if name == "big-smallest":
        assert kinds == {2} and P.n_fronts == 1
    if name == "big":
        assert {4, 2} <= kinds and 3 not in kinds
    if name == "big-wide":
        assert {2, 3} <= kinds
    if name.endswith("-shared"):
        assert S["n_shared"] > 0
    # leaf instance, bottom subtrees, four-wave block: whole levels, consistent with each other
    os_ = S["own_start"]; total = int(os_[-1])
    assert 0 <= S["leaf_n"] <= os_[1] and S["block_n"] >= 0
    assert total - S["block_n"] in os_.tolist() or S["block_n"] == total - max(S["leaf_n"], S["sub_first"] + S["n_subtrees"])
    if name in ("lap", "bench1000"):                             # few leaves (<= leaf_min = 2048): the whole-tree launch takes level 0 as well
        assert S["leaf_n"] == 0 and S["n_subtrees"] == 0 and S["bs_l0"] == 0
        assert [int(r[0]) for r in S["launches_tree"]] == [K_TREE, K_BTREE]
        assert all(int(r[0]) in (K_LEVEL, K_BLEVEL) for r in S["launches_level"]) and len(S["launches_level"]) == 2 * S["n_levels"]
    if name in ("lap-leaf0", "bench1000-leaf0"):                 # the leaf instance; the bottom subtrees if the plan qualifies
        assert S["leaf_n"] == os_[1] > 0 and S["bs_l0"] >= 1
        if S["n_subtrees"] > 0:
            assert S["sub_first"] == os_[1] and S["n_subtrees"] == os_[2] - os_[1] and 0 <= S["sub_free"] <= S["leaf_n"]
            for q in range(S["leaf_n"]):                         # leaves behind sub_free hang under a level-1 front, the ones before do not
                pa = int(P.parent[S["own_fronts"][q]])
                assert (pa >= 0 and P.level[pa] == 1) == (q >= S["sub_free"])
            assert S["launches_tree"][0][3] > 0                  # the subtree workgroups' LDS is the schedule's
        else:
            assert S["sub_free"] == S["leaf_n"] and S["sub_first"] == 0
        print("%s: leaf_n %d n_subtrees %d sub_free %d block_n %d bs_l0 %d" % (name, S["leaf_n"], S["n_subtrees"], S["sub_free"], S["block_n"], S["bs_l0"]))


@pytest.mark.parametrize("name", ["lap-leaf0", "big", "big-shared"])
def test_the_schedule_has_no_history(pkg, bench_graphs, frontend, case, name):
    S, _ = case(name)
    G = handle(pkg, bench_graphs, frontend, name)
    a = G.debug_schedule()["raw"]; b = G.debug_schedule()["raw"]; G.close()
    assert np.array_equal(a, b) and np.array_equal(a, S["raw"])      # twice on one handle; a second handle with the same graph
