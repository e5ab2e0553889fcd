"""CPU tests of the minimum-cost association: the header declares and the library exports it, the host-side refusals on a host-only handle,
the two exact statements of the rule in assign_opt_ref.py (the enumeration of all matchings and successive shortest paths) against each
other and against the greedy matching, the smallest case that separates the two rules, and the census of the 55 frames that the cases of
assoc_nn_shapes.py give when grouped by pose — from the exact reference alone.  Nothing here runs a kernel."""
import ctypes as C

import numpy as np
import pytest

import assign_nn_ref as ar
import assign_opt_ref as ao
import assoc_nn_shapes as ns

NEW_FUNCS = ("gs_assign_opt_batch", "gs_assign_opt_resident", "gs_frame_frontend_assign_opt", "gs_debug_time_assign_opt_resident")
SEPARATING = [[1.0, 2.0], [1.5, ao.INF]]                                     # the greedy takes (0, 0) and leaves observation 1 without a cone
GATE = 5.99


def test_the_header_declares_and_the_library_exports(pkg):
    names = pkg.binding.declared_symbols(); L = pkg.binding.lib()
    for f in NEW_FUNCS:
        assert f in names, f
        assert hasattr(L, f), f
    assert "#define GS_ASSIGN_CAND_MAX 8" in open(pkg.binding.HEADER).read()
    for f in ("assign_opt", "assign_opt_resident", "frame_frontend_assign_opt", "time_assign_opt_resident"):
        assert hasattr(pkg.Graph, f), f


def test_refusals_on_a_host_only_handle(pkg):
    b = pkg.binding; L = b.lib(); G = pkg.Graph(device=-2)
    poses = np.zeros((1, 3)); po = np.zeros(2, dtype=np.int32); ob = np.array([[10.0, 0, 5, 1], [20.0, 0, 6, 2]]); xy = np.ones((3, 2)); ty = np.ones(3, dtype=np.int32)
    fs = np.array([0, 1, 2], dtype=np.int32)
    def code(fn, *a, **kw):
        with pytest.raises(b.GsError) as e:
            fn(*a, **kw)
        return e.value.code
    bad = [dict(gate_chi2=0.0), dict(gate_chi2=-1.0), dict(max_distance=0.0), dict(max_distance=-3.0), dict(sigma_range=-1e-9), dict(sigma_bearing=-1.0),
           dict(sigma_xy=-0.05), dict(struct_size=48), dict(struct_size=0)]
    bad += [{k: v} for k in ("gate_chi2", "max_distance", "type_tol", "sigma_range", "sigma_bearing", "sigma_xy") for v in (float("nan"), float("inf"), -float("inf"))]
    da = C.c_void_p(4096)                                                    # never dereferenced: every refusal below is decided on the host
    for kw in bad:
        prm = b.nn_params(**kw)
        assert code(G.assign_opt, poses, po, ob, fs, xy, ty, params=prm) == -1, kw
        assert code(G.frame_frontend_assign_opt, poses[0], ob, params=prm) == -1, kw
        assert L.gs_assign_opt_resident(G.h, 2, da, 1, da, da, 2, da, None, C.byref(prm), da, None, None) == -1, kw
    prm = b.nn_params()
    assert code(G.assign_opt, poses, po, ob, fs, xy, ty) == -4 and code(G.frame_frontend_assign_opt, poses[0], ob) == -4     # good arguments: GS_ERR_NO_DEVICE
    assert code(G.assign_opt, poses, po, ob, [0, 0, 2, 2], xy, ty) == -4                                                      # empty frames are allowed
    res = lambda **kw: L.gs_assign_opt_resident(*[kw.get(k, v) for k, v in (("g", G.h), ("n", 2), ("p", da), ("np", 1), ("po", da), ("ob", da), ("nf", 2), ("fs", da),
                                                                              ("pc", None), ("prm", C.byref(prm)), ("out", da), ("d2", None), ("na", None))])
    assert res() == -4 and res(na=da, d2=da) == -4
    assert res(ob=C.c_void_p(4096 + 8)) == -1                                                                                 # dev_obs not 32-byte aligned
    for k in ("g", "p", "po", "ob", "fs", "prm", "out"):
        assert res(**{k: None}) == -1, k
    assert res(n=-1) == -1 and res(nf=-1) == -1 and res(np=-1) == -1
    assert code(G.assign_opt, poses, np.array([0, 1], dtype=np.int32), ob, fs, xy, ty) == -1                                  # pose_of_obs out of range
    # frame_start (the check the greedy calls use): first != 0, descending, last != n, a frame of 257
    for f in ([1, 1, 2], [0, 2, 1, 2], [0, 1, 1], [0, 1, 3], [0, 2, 1]):
        assert code(G.assign_opt, poses, po, ob, f, xy, ty) == -1, f
        assert code(G.assign_nn, poses, po, ob, f, xy, ty) == -1, f
    big = np.tile(ob[:1], (300, 1)); pob = np.zeros(300, dtype=np.int32)
    assert code(G.assign_opt, poses, pob, big, [0, 257, 300], xy, ty) == -1
    assert code(G.assign_opt, poses, pob, big, [0, 43, 300], xy, ty) == -1
    assert code(G.assign_opt, poses, pob, big, [0, 44, 300], xy, ty) == -4                                                     # 44 + 256
    assert code(G.frame_frontend_assign_opt, poses[0], big[:257]) == -1 and code(G.frame_frontend_assign_opt, poses[0], big[:256]) == -4
    dp = C.POINTER(C.c_double); ip = C.POINTER(C.c_int32); out = np.zeros(2, dtype=np.int32)
    args = lambda **kw: [kw.get(k, v) for k, v in (("g", G.h), ("n", 2), ("poses", poses.ctypes.data_as(dp)), ("np", 1), ("po", po.ctypes.data_as(ip)),
                                                   ("ob", ob.ctypes.data_as(dp)), ("nf", 2), ("fs", fs.ctypes.data_as(ip)), ("m", 3), ("xy", xy.ctypes.data_as(dp)),
                                                   ("ty", ty.ctypes.data_as(ip)), ("mc", None), ("pc", None), ("prm", C.byref(prm)), ("out", out.ctypes.data_as(ip)), ("d2", None),
                                                   ("na", None))]
    assert L.gs_assign_opt_batch(*args()) == -4
    for k in ("g", "poses", "po", "ob", "fs", "xy", "ty", "prm", "out"):
        assert L.gs_assign_opt_batch(*args(**{k: None})) == -1, k
    assert L.gs_assign_opt_batch(*args(n=-1)) == -1 and L.gs_assign_opt_batch(*args(m=-1)) == -1 and L.gs_assign_opt_batch(*args(nf=-1)) == -1
    z = np.zeros(4); i2 = np.zeros(2, dtype=np.int32)
    fa = lambda **kw: [kw.get(k, v) for k, v in (("g", G.h), ("pose", poses.ctypes.data_as(dp)), ("pc", None), ("ob", ob.ctypes.data_as(dp)), ("k", 2), ("prm", C.byref(prm)),
                                                 ("z", z.ctypes.data_as(dp)), ("gx", z.ctypes.data_as(dp)), ("i", i2.ctypes.data_as(ip)), ("d2", z.ctypes.data_as(dp)), ("na", None))]
    assert L.gs_frame_frontend_assign_opt(*fa()) == -4 and L.gs_frame_frontend_assign_opt(*fa(na=i2.ctypes.data_as(ip))) == -4
    for k in ("g", "pose", "ob", "prm", "z", "gx", "i", "d2"):
        assert L.gs_frame_frontend_assign_opt(*fa(**{k: None})) == -1, k
    assert L.gs_frame_frontend_assign_opt(*fa(k=-1)) == -1
    ms = C.c_double()
    assert L.gs_debug_time_assign_opt_resident(G.h, 2, da, 1, da, da, 2, da, None, C.byref(prm), da, None, None, 0, C.byref(ms)) == -1
    assert L.gs_debug_time_assign_opt_resident(G.h, 2, da, 1, da, da, 2, da, None, C.byref(prm), da, None, None, 3, C.byref(ms)) == -4
    G.close()


def test_the_smallest_separating_case():
    rows = ao.cut(ao.rows_of(SEPARATING))
    g_idx, g_d2 = ar.greedy(SEPARATING)
    assert g_idx == [0, -1] and ao.value(rows, g_idx, GATE) == ao.frac(GATE) - 1
    for best, idx in (ao.enumerate_best(rows, GATE), ao.solve(rows, GATE)):
        assert idx == [1, 0] and best == 2 * ao.frac(GATE) - ao.frac(3.5)
    assert ao.margin(rows, GATE) == (2 * ao.frac(GATE) - ao.frac(3.5)) - (ao.frac(GATE) - 1)       # the best different matching is the greedy's


def test_the_two_statements_agree_and_beat_the_greedy_on_random_matrices_with_ties():
    """small integer distances (scaled, so that they are not integers in binary), a third of the pairs not admissible, up to 6 x 6"""
    rng = np.random.default_rng(7); better = ties = 0
    for t in range(3000):
        k, m = rng.integers(1, 7), rng.integers(1, 7); scale = 1.0 if t % 2 else 0.37
        D = rng.integers(1, 6, (k, m)).astype(np.float64) * scale; D[rng.uniform(size=(k, m)) < 0.33] = np.inf
        gate = 5.99 if t % 3 else 4.0 * scale
        D[D >= gate] = np.inf                                                # (admissible means d2 < gate)
        rows = ao.cut(ao.rows_of(D))
        be, me = ao.enumerate_best(rows, gate); bs, ms = ao.solve(rows, gate)
        assert be == bs, (t, D.tolist(), me, ms)
        assert ao.value(rows, me, gate) == be and ao.value(rows, ms, gate) == bs
        gv = ao.value(rows, ar.greedy(D)[0], gate)
        assert gv <= be, (t, D.tolist())
        better += gv < be
        mg = ao.margin(rows, gate); ties += mg == 0
        if mg > 0:
            assert me == ms, (t, D.tolist())                                 # a unique optimum: both statements return it
        for a, j in enumerate(ms):                                           # maximal: no observation at -1 with a free cone on its list
            assert j != -1 or all(c in ms for _, c in rows[a]), (t, D.tolist(), ms)
    print("the optimum beats the greedy on %d of 3000 matrices; %d have two optima" % (better, ties))
    assert better > 100 and ties > 100


def test_the_cut_to_eight_candidates():
    """an observation with 9 admissible cones whose 8 nearest are each the only candidate of another observation keeps none: the 9th is cut"""
    D = np.full((9, 9), np.inf); D[0] = 1.0 + 0.1 * np.arange(9)
    for i in range(1, 9):
        D[i, i - 1] = 0.5
    rows = ao.cut(ao.rows_of(D)); assert len(rows[0]) == 8 and 8 not in [j for _, j in rows[0]]
    best, idx = ao.solve(rows, GATE)
    assert idx == [-1] + list(range(8)) and best == 8 * (ao.frac(GATE) - ao.frac(0.5))
    assert ao.solve(ao.rows_of(D), GATE)[1] == [8] + list(range(8))          # without the cut it would take the 9th


@pytest.fixture(scope="module")
def census():
    """per case: (order, frame_start, [FrameRef]) with frames = the observations grouped by pose"""
    out = {}
    for name in ns.NAMES:
        c = ns.case(name); R = ns.reference(name)
        order, fs = ar.frames_by_pose(c["pose_of"])
        out[name] = (order, fs, [ao.FrameRef(R, order[fs[f]:fs[f + 1]]) for f in range(len(fs) - 1)])
    return out


def test_census_every_frame_is_decided_and_the_greedy_loses_in_many(census):
    lines = []; frames = undecided = loses = cut = most = 0; least = None
    for name, (order, fs, F) in census.items():
        for n, f in enumerate(F):
            gi, gv = f.greedy(); frames += 1; undecided += not f.decided; lose = gv < f.best; loses += lose
            assert gv <= f.best
            assert lose or f.margin == 0 or gi == f.expect                   # equal totals and a unique optimum: the same matching
            most = max([most] + f.n_poss); cut += sum(p > ao.CAND_MAX for p in f.n_poss)
            bound = f.T + 2 * f.sum_b
            if f.margin != ao.INF:
                least = f.margin if least is None else min(least, f.margin)
            lines.append("%-16s frame %d: k %3d pairs %4d decided %d optimum %.6f greedy %.6f margin %.3e T + 2 sum B %.3e" % (
                name, n, f.k, sum(len(r) for r in f.rows), f.decided, float(f.best), float(gv), float(f.margin), float(bound)))
    lines.append("frames %d undecided %d greedy loses %d observations cut %d most admissible %d least margin %.3e" % (frames, undecided, loses, cut, most, float(least)))
    print("\n".join(lines))                                                  # (profiles/assign_opt_cpu_census.txt is this print)
    assert frames == 55
    assert undecided == 0
    assert loses >= 10


def test_the_checker_has_teeth(census):
    """the exact optimum passes; the greedy where it loses, a doubly used cone, a -1 where a free cone remains, a d2 off by 3 B and a wrong
    count are each rejected"""
    n = lost = 0
    for name in ("map2047", "grid_nonfinite", "k64", "k65", "grid_crowd"):
        for f in census[name][2]:
            idx = list(f.expect); d2 = [float(f.pairs[(a, j)].d2) if j >= 0 else ao.INF for a, j in enumerate(idx)]
            assert not f.failures(idx, d2, f.n_poss), (name, f.failures(idx, d2, f.n_poss)[:2])
            gi, gv = f.greedy()
            if gv < f.best:
                gd = [float(f.pairs[(a, j)].d2) if j >= 0 else ao.INF for a, j in enumerate(gi)]
                assert any("exact optimum" in w for _, w in f.failures(gi, gd)), "the greedy where it loses"; lost += 1
            got = [a for a, j in enumerate(idx) if j >= 0]
            if len(got) < 2:
                continue
            a, b = got[0], got[-1]
            s = list(idx); s[b] = idx[a]; sd = list(d2); sd[b] = d2[a]
            assert any("twice" in w for _, w in f.failures(s, sd)), "a doubly used cone"
            s = list(idx); s[a] = -1; sd = list(d2); sd[a] = ao.INF
            assert any(p == a and "remains free" in w for p, w in f.failures(s, sd)), "-1 where a free cone remains"
            sd = list(d2); sd[a] = float(d2[a] + 3 * float(f.pairs[(a, idx[a])].B))
            assert [p for p, _ in f.failures(idx, sd)] == [a], "d2 off by 3 B"
            na = list(f.n_poss); na[a] += 1
            assert [p for p, _ in f.failures(idx, d2, na)] == [a], "a wrong count"
            n += 1
    assert n >= 5 and lost >= 3
