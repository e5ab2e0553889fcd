"""CPU tests of the one-to-one association: the header declares and the library exports it, the host-side refusals on a host-only handle,
the two statements of the rule in assign_nn_ref.py (the sorted greedy walk and the mutual-best rounds) against each other, that the checker
has teeth, and the census of what the cases of assoc_nn_shapes.py reach when their observations are grouped into frames by pose — from the
exact reference alone.  Nothing here runs a kernel."""
import ctypes as C

import numpy as np
import pytest

import assign_nn_ref as ar
import assoc_nn_shapes as ns

NEW_FUNCS = ("gs_assign_nn_batch", "gs_assign_nn_resident", "gs_frame_frontend_assign", "gs_debug_time_assign_nn_resident")
TRAP = [[0.5, ar.INF], [1.0, 2.0], [ar.INF, 3.0]]                            # the smallest matrix that separates the rule from the proposer-only shortcut


def test_the_header_declares_and_the_library_exports(pkg):
    names = pkg.binding.declared_symbols(); L = pkg.binding.lib()
    for f in NEW_FUNCS:
        assert f in names, f
        assert hasattr(L, f), f
    assert "#define GS_NN_FRAME_MAX 256" in open(pkg.binding.HEADER).read()


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
        assert code(G.assign_nn, poses, po, ob, fs, xy, ty, params=prm) == -1, kw
        assert code(G.frame_frontend_assign, poses[0], ob, params=prm) == -1, kw
        assert L.gs_assign_nn_resident(G.h, 2, da, 1, da, da, 2, da, None, C.byref(prm), da, None) == -1, kw
    prm = b.nn_params()
    assert code(G.assign_nn, poses, po, ob, fs, xy, ty) == -4 and code(G.frame_frontend_assign, poses[0], ob) == -4       # good arguments: GS_ERR_NO_DEVICE
    assert code(G.assign_nn, poses, po, ob, [0, 0, 2, 2], xy, ty) == -4                                                    # empty frames are allowed
    res = lambda **kw: L.gs_assign_nn_resident(*[kw.get(k, v) for k, v in (("g", G.h), ("n", 2), ("p", da), ("np", 1), ("po", da), ("ob", da), ("nf", 2), ("fs", da),
                                                                             ("pc", None), ("prm", C.byref(prm)), ("out", da), ("d2", None))])
    assert res() == -4
    assert res(ob=C.c_void_p(4096 + 8)) == -1                                                                              # dev_obs not 32-byte aligned
    for k in ("g", "p", "po", "ob", "fs", "prm", "out"):
        assert res(**{k: None}) == -1, k
    assert res(n=-1) == -1 and res(nf=-1) == -1 and res(np=-1) == -1
    assert code(G.assign_nn, poses, np.array([0, 1], dtype=np.int32), ob, fs, xy, ty) == -1                                # pose_of_obs out of range
    # frame_start: first != 0, descending, last != n, a frame of 257
    for f in ([1, 1, 2], [0, 2, 1, 2], [0, 1, 1], [0, 1, 3], [0, 2, 1]):
        assert code(G.assign_nn, poses, po, ob, f, xy, ty) == -1, f
    big = np.tile(ob[:1], (300, 1)); pob = np.zeros(300, dtype=np.int32)
    assert code(G.assign_nn, poses, pob, big, [0, 257, 300], xy, ty) == -1
    assert code(G.assign_nn, poses, pob, big, [0, 43, 300], xy, ty) == -1
    assert code(G.assign_nn, poses, pob, big, [0, 44, 300], xy, ty) == -4                                                   # 44 + 256
    assert code(G.frame_frontend_assign, poses[0], big[:257]) == -1 and code(G.frame_frontend_assign, poses[0], big[:256]) == -4
    dp = C.POINTER(C.c_double); ip = C.POINTER(C.c_int32); out = np.zeros(2, dtype=np.int32)
    args = lambda **kw: [kw.get(k, v) for k, v in (("g", G.h), ("n", 2), ("poses", poses.ctypes.data_as(dp)), ("np", 1), ("po", po.ctypes.data_as(ip)),
                                                   ("ob", ob.ctypes.data_as(dp)), ("nf", 2), ("fs", fs.ctypes.data_as(ip)), ("m", 3), ("xy", xy.ctypes.data_as(dp)),
                                                   ("ty", ty.ctypes.data_as(ip)), ("mc", None), ("pc", None), ("prm", C.byref(prm)), ("out", out.ctypes.data_as(ip)), ("d2", None))]
    assert L.gs_assign_nn_batch(*args()) == -4
    for k in ("g", "poses", "po", "ob", "fs", "xy", "ty", "prm", "out"):
        assert L.gs_assign_nn_batch(*args(**{k: None})) == -1, k
    assert L.gs_assign_nn_batch(*args(n=-1)) == -1 and L.gs_assign_nn_batch(*args(m=-1)) == -1 and L.gs_assign_nn_batch(*args(nf=-1)) == -1
    z = np.zeros(4); i2 = np.zeros(2, dtype=np.int32)
    fa = lambda **kw: [kw.get(k, v) for k, v in (("g", G.h), ("pose", poses.ctypes.data_as(dp)), ("pc", None), ("ob", ob.ctypes.data_as(dp)), ("k", 2), ("prm", C.byref(prm)),
                                                 ("z", z.ctypes.data_as(dp)), ("gx", z.ctypes.data_as(dp)), ("i", i2.ctypes.data_as(ip)), ("d2", z.ctypes.data_as(dp)))]
    assert L.gs_frame_frontend_assign(*fa()) == -4
    for k in ("g", "pose", "ob", "prm", "z", "gx", "i", "d2"):
        assert L.gs_frame_frontend_assign(*fa(**{k: None})) == -1, k
    assert L.gs_frame_frontend_assign(*fa(k=-1)) == -1
    ms = C.c_double()
    assert L.gs_debug_time_assign_nn_resident(G.h, 2, da, 1, da, da, 2, da, None, C.byref(prm), da, None, 0, C.byref(ms)) == -1
    assert L.gs_debug_time_assign_nn_resident(G.h, 2, da, 1, da, da, 2, da, None, C.byref(prm), da, None, 3, C.byref(ms)) == -4
    G.close()


def test_the_trap_separates_the_rule_from_the_shortcut():
    assert ar.greedy(TRAP)[0] == [0, 1, -1] and ar.greedy(TRAP)[1] == [0.5, 2.0, ar.INF]
    assert ar.mutual_best(TRAP)[:2] == ar.greedy(TRAP)
    assert ar.mutual_best(TRAP, proposers_only=True)[0] == [0, -1, 1]


def test_greedy_and_mutual_best_agree_on_random_matrices_with_ties():
    """small integer distances, so exact ties are everywhere; a third of the pairs not admissible"""
    rng = np.random.default_rng(5); differ = 0; most = 0
    for t in range(2000):
        k, m = rng.integers(1, 9), rng.integers(1, 9)
        D = rng.integers(1, 6, (k, m)).astype(np.float64); D[rng.uniform(size=(k, m)) < 0.33] = np.inf
        a = ar.greedy(D); b = ar.mutual_best(D); most = max(most, b[2])
        assert a[0] == b[0] and a[1] == b[1], (t, D.tolist(), a, b)
        assert b[2] <= k                                                     # a round commits at least the smallest open pair
        assert not ar.has_duplicates(a[0])
        differ += ar.mutual_best(D, proposers_only=True)[0] != a[0]
    print("the proposer-only shortcut differs on %d of 2000 matrices; most rounds %d" % (differ, most))
    assert differ > 20


@pytest.fixture(scope="module")
def census():
    """per case: (order, frame_start, [FrameRef]) with frames = the observations grouped by pose"""
    out = {}
    for name in ns.NAMES:
        c = ns.case(name); R = ns.reference(name)
        order, fs = ar.frames_by_pose(c["pose_of"])
        out[name] = (order, fs, [ar.FrameRef(R, order[fs[f]:fs[f + 1]]) for f in range(len(fs) - 1)])
    return out


def test_census_every_frame_is_decided_and_many_are_contested(census):
    frames = contested = undecided = largest = 0
    for name, (order, fs, F) in census.items():
        assert fs[0] == 0 and fs[-1] == len(ns.case(name)["obs"]) and (np.diff(fs) <= 256).all(), name
        for f in F:
            frames += 1; contested += f.contested; undecided += not f.decided; largest = max(largest, len(f.members))
        print("%-16s frames %d sizes %s contested %d cones %s" % (name, len(F), np.diff(fs).tolist(), sum(f.contested for f in F), [len(f.cones) for f in F]))
    print("frames %d contested %d undecided %d largest %d" % (frames, contested, undecided, largest))
    assert undecided == 0
    assert contested >= 20
    assert frames >= 50 and largest >= 128


def test_the_checker_has_teeth(census):
    """the exact greedy passes; swapping two observations' cones, a doubly used cone, and a -1 where a free sure cone remains are each rejected"""
    n = 0
    for name in ("map257", "random2048", "k65"):
        for f in census[name][2]:
            idx = list(f.expect); d2 = [float(f.pairs[(a, j)].d2) if j >= 0 else ar.INF for a, j in enumerate(idx)]
            assert not f.failures(idx, d2), (name, f.failures(idx, d2)[:2])
            got = [a for a, j in enumerate(idx) if j >= 0]
            if len(got) < 2:
                continue
            a, b = got[0], got[-1]
            s = list(idx); s[a], s[b] = s[b], s[a]; sd = list(d2); sd[a], sd[b] = sd[b], sd[a]
            assert {p for p, _ in f.failures(s, sd)} >= {a, b}, "swapped cones"
            s = list(idx); s[b] = idx[a]; sd = list(d2); sd[b] = d2[a]
            assert any("twice" in w for _, w in f.failures(s, sd)), "a doubly used cone"
            s = list(idx); s[a] = -1; sd = list(d2); sd[a] = ar.INF
            assert any(p == a and "remains free" in w for p, w in f.failures(s, sd)), "-1 where a free sure cone remains"
            sd = list(d2); sd[a] = float(d2[a] + 3 * float(f.pairs[(a, idx[a])].B))
            assert [p for p, _ in f.failures(idx, sd)] == [a], "d2 off by 3 B"
            n += 1
    assert n >= 5
