"""CPU tests of the joint compatibility test: the header declares and the library exports it, the gate table against mpmath's regularised
gamma function, every host-side refusal on a host-only handle, the exact reference (joint_compat_ref.py) against the dense
nu^T S^-1 nu in mpmath, and the census of the purpose-made scenes (joint_compat_shapes.py): every frame DECIDED by the reference alone, each
scene doing what it was made for.  Nothing here runs a kernel."""
import ctypes as C
import math

import numpy as np
import pytest

import joint_compat_ref as jr
import joint_compat_shapes as js

NEW_FUNCS = ("gs_jc_params_default", "gs_jc_params_set_confidence", "gs_joint_compat_batch", "gs_joint_compat_resident", "gs_frame_frontend_jc",
             "gs_debug_time_joint_compat_resident")


def test_the_header_declares_and_the_library_exports(pkg):
    names = pkg.binding.declared_symbols(); L = pkg.binding.lib()
    for f in NEW_FUNCS:
        assert f in names, f
        assert hasattr(L, f), f
    for f in ("joint_compat", "joint_compat_resident", "frame_frontend_jc", "time_joint_compat_resident"):
        assert hasattr(pkg.Graph, f), f
    assert C.sizeof(pkg.binding.JcParams) == 16 + 8 * 257 and pkg.binding.jc_params().struct_size == C.sizeof(pkg.binding.JcParams)


def test_the_default_gate_table(pkg):
    p = pkg.binding.jc_params(); g = np.array(p.gate)
    assert p.confidence == 0.95 and len(g) == 257 and g[0] == 0.0
    assert abs(g[1] - (-2.0 * math.log(0.05))) <= 1e-12 * (-2.0 * math.log(0.05))
    assert (np.diff(g) >= 0).all() and np.isfinite(g).all()
    for m in (1, 2, 3, 64, 256):
        assert abs(jr.chi2_cdf(m, g[m]) - 0.95) <= 1e-12, (m, g[m])
    q = pkg.binding.jc_params(confidence=0.5); h = np.array(q.gate)
    assert q.confidence == 0.5 and h[0] == 0.0 and (np.diff(h) >= 0).all() and (h[1:] < g[1:]).all()
    for m in (1, 7, 256):
        assert abs(jr.chi2_cdf(m, h[m]) - 0.5) <= 1e-12, m
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(pkg.binding.GsError) as e:
            pkg.binding.jc_params(confidence=bad)
        assert e.value.code == -1, bad
    assert pkg.binding.lib().gs_jc_params_default(None) == -1


def test_refusals_on_a_host_only_handle(pkg):
    b = pkg.binding; L = b.lib(); G = pkg.Graph(device=-2)
    poses = np.zeros((2, 3)); po = np.zeros(2, dtype=np.int32); ob = np.array([[10.0, 0, 5, 1], [20.0, 0, 6, 2]]); xy = np.ones((3, 2))
    fs = np.array([0, 1, 2], dtype=np.int32); hyp = np.array([2, -1], dtype=np.int32)
    def code(fn, *a, **kw):
        with pytest.raises(b.GsError) as e:
            fn(*a, **kw)
        return e.value.code
    da = C.c_void_p(4096)                                                    # never dereferenced: every refusal below is decided on the host
    prm = b.nn_params(); jc = b.jc_params()
    res = lambda **kw: L.gs_joint_compat_resident(*[kw.get(k, v) for k, v in (("g", G.h), ("n", 2), ("p", da), ("np", 1), ("po", da), ("ob", da), ("nf", 2), ("fs", da),
                                                                                ("pc", None), ("prm", C.byref(prm)), ("jc", C.byref(jc)), ("in", da), ("out", da), ("j", None),
                                                                                ("nk", None), ("nd", None), ("nu", None), ("dl", None))])
    # good arguments: GS_ERR_NO_DEVICE; the per-frame outputs are optional
    assert code(G.joint_compat, poses, po, ob, fs, xy, hyp) == -4 and code(G.frame_frontend_jc, poses[0], ob) == -4
    assert code(G.joint_compat, poses, po, ob, [0, 0, 2, 2], xy, hyp) == -4                                                   # empty frames are allowed
    assert res() == -4 and res(j=da, nk=da, nd=da, nu=da, dl=da, pc=da) == -4
    # the sigmas (the only fields of gs_nn_params the joint test reads) and struct_size
    bad = [dict(sigma_range=-1e-9), dict(sigma_bearing=-1.0), dict(sigma_xy=-0.05), dict(struct_size=48), dict(struct_size=0)]
    bad += [{k: v} for k in ("sigma_range", "sigma_bearing", "sigma_xy") for v in (float("nan"), float("inf"), -float("inf"))]
    for kw in bad:
        p = b.nn_params(**kw)
        assert code(G.joint_compat, poses, po, ob, fs, xy, hyp, params=p) == -1, kw
        assert code(G.frame_frontend_jc, poses[0], ob, params=p) == -1, kw
        assert res(prm=C.byref(p)) == -1, kw
    for kw in (dict(gate_chi2=-1.0), dict(max_distance=0.0), dict(type_tol=float("nan"))):                                    # not read by the batch and resident calls ...
        p = b.nn_params(**kw)
        assert code(G.joint_compat, poses, po, ob, fs, xy, hyp, params=p) == -4 and res(prm=C.byref(p)) == -4, kw
        assert code(G.frame_frontend_jc, poses[0], ob, params=p) == -1, kw                                                    # ... but by the frame call's assignment
    # the table
    def table(**kw):
        t = b.jc_params()
        for k, v in kw.items():
            if k == "struct_size":
                t.struct_size = v
            else:
                t.gate[int(k[1:])] = v
        return t
    for kw in (dict(struct_size=0), dict(struct_size=2072 + 8), dict(g5=float("nan")), dict(g256=float("inf")), dict(g0=-1.0), dict(g3=-0.5), dict(g7=1.0),
               dict(g255=1e9)):
        t = table(**kw)
        assert code(G.joint_compat, poses, po, ob, fs, xy, hyp, jc=t) == -1, kw
        assert code(G.frame_frontend_jc, poses[0], ob, jc=t) == -1, kw
        assert res(jc=C.byref(t)) == -1, kw
    t = table(g0=1.0, g1=1.0); t.confidence = float("nan")                                                                     # an edited table is the caller's right
    assert code(G.joint_compat, poses, po, ob, fs, xy, hyp, jc=t) == -4 and res(jc=C.byref(t)) == -4
    # pointers, counts, alignment (resident)
    assert res(ob=C.c_void_p(4096 + 8)) == -1                                                                                 # dev_obs not 32-byte aligned
    for k in ("g", "p", "po", "ob", "fs", "prm", "jc", "in", "out"):
        assert res(**{k: None}) == -1, k
    assert res(n=-1) == -1 and res(nf=-1) == -1 and res(np=-1) == -1
    # the hypothesis, the pose indices, the frames (batch)
    for h in ([3, -1], [-2, 0], [0, 2 ** 30]):
        assert code(G.joint_compat, poses, po, ob, fs, xy, h) == -1, h
    assert code(G.joint_compat, poses, po, ob, fs, xy, [2, 2]) == -4                                                          # a cone named twice is not checked
    assert code(G.joint_compat, poses, np.array([0, 2], dtype=np.int32), ob, fs, xy, hyp) == -1                               # pose_of_obs out of range
    assert code(G.joint_compat, poses, np.array([0, 1], dtype=np.int32), ob, [0, 2], xy, hyp) == -1                           # a frame with two poses
    assert code(G.joint_compat, poses, np.array([0, 1], dtype=np.int32), ob, fs, xy, hyp) == -4                               # ... in two frames: fine
    for f in ([1, 1, 2], [0, 2, 1, 2], [0, 1, 1], [0, 1, 3], [0, 2, 1]):
        assert code(G.joint_compat, poses, po, ob, f, xy, hyp) == -1, f
    big = np.tile(ob[:1], (300, 1)); pob = np.zeros(300, dtype=np.int32); hb = np.full(300, -1, dtype=np.int32)
    assert code(G.joint_compat, poses, pob, big, [0, 257, 300], xy, hb) == -1
    assert code(G.joint_compat, poses, pob, big, [0, 44, 300], xy, hb) == -4                                                   # 44 + 256
    assert code(G.frame_frontend_jc, poses[0], big[:257]) == -1 and code(G.frame_frontend_jc, poses[0], big[:256]) == -4
    dp = C.POINTER(C.c_double); ip = C.POINTER(C.c_int32); out = np.zeros(2, dtype=np.int32)
    args = lambda **kw: [kw.get(k, v) for k, v in (("g", G.h), ("n", 2), ("poses", poses.ctypes.data_as(dp)), ("np", 2), ("po", po.ctypes.data_as(ip)),
                                                   ("ob", ob.ctypes.data_as(dp)), ("nf", 2), ("fs", fs.ctypes.data_as(ip)), ("m", 3), ("xy", xy.ctypes.data_as(dp)),
                                                   ("mc", None), ("pc", None), ("prm", C.byref(prm)), ("jc", C.byref(jc)), ("in", hyp.ctypes.data_as(ip)),
                                                   ("out", out.ctypes.data_as(ip)), ("j", None), ("nk", None), ("nd", None), ("nu", None), ("dl", None))]
    assert L.gs_joint_compat_batch(*args()) == -4
    for k in ("g", "poses", "po", "ob", "fs", "xy", "prm", "jc", "in", "out"):
        assert L.gs_joint_compat_batch(*args(**{k: None})) == -1, k
    assert L.gs_joint_compat_batch(*args(n=-1)) == -1 and L.gs_joint_compat_batch(*args(m=-1)) == -1 and L.gs_joint_compat_batch(*args(nf=-1)) == -1
    z = np.zeros(4); i2 = np.zeros(2, dtype=np.int32)
    fa = lambda **kw: [kw.get(k, v) for k, v in (("g", G.h), ("pose", poses.ctypes.data_as(dp)), ("pc", None), ("ob", ob.ctypes.data_as(dp)), ("k", 2), ("prm", C.byref(prm)),
                                                 ("jc", C.byref(jc)), ("z", z.ctypes.data_as(dp)), ("gx", z.ctypes.data_as(dp)), ("i", i2.ctypes.data_as(ip)),
                                                 ("d2", z.ctypes.data_as(dp)), ("na", None), ("j", None), ("nk", None), ("nd", None), ("nu", None), ("dl", None))]
    assert L.gs_frame_frontend_jc(*fa()) == -4
    for k in ("g", "pose", "ob", "prm", "jc", "z", "gx", "i", "d2"):
        assert L.gs_frame_frontend_jc(*fa(**{k: None})) == -1, k
    assert L.gs_frame_frontend_jc(*fa(k=-1)) == -1
    ms = C.c_double()
    tm = lambda reps: L.gs_debug_time_joint_compat_resident(G.h, 2, da, 1, da, da, 2, da, None, C.byref(prm), C.byref(jc), da, da, None, None, None, None, None, reps, C.byref(ms))
    assert tm(0) == -1 and tm(3) == -4
    G.close()


@pytest.fixture(scope="module")
def census(pkg):
    """(scene, regime) -> the eliminated FrameRef, from the library's own table of the scene's confidence"""
    out = {}
    for name, reg in js.NAMES:
        c = js.scene(name, reg)
        out[(name, reg)] = jr.make(c, c["hyp"], c["frame_start"], list(pkg.binding.jc_params(c["confidence"]).gate))[0].eliminate()
    return out


def test_the_reference_against_the_dense_solve(census):
    """J of every subset the elimination met, and of a few more, against nu^T (blockdiag(D) + G Sigma_p G^T)^-1 nu in mpmath"""
    worst = 0
    for key, F in census.items():
        sets = [sorted(F.pairs), F.kept, [0], [1, 6], [0, 2, 3, 5, 7]] + [[a for a in sorted(F.pairs) if a not in F.order[:t]] for t in range(len(F.order))]
        for K in sets:
            J = F.J_of(K)[0]; d = jr.brute(F, K)
            assert abs(J - d) <= 1e-40 * max(1, abs(d)), (key, K, float(J), float(d))
            worst = max(worst, float(abs(J - d)))
    print("largest |Woodbury - dense| %.3g" % worst)


def test_census_every_frame_is_decided_and_does_what_it_was_made_for(census):
    lines = []
    for (name, reg), F in census.items():
        lines.append("%-12s %s kept %s left %s rounds %d J %.12g B %.3g gate %.6g delta (%.6g, %.6g, %.6g) least margin %.3g B decided %d" % (
            name, reg, F.kept, F.order, F.rounds, float(F.J), float(F.B), F.gate[len(F.kept)], *[float(d) for d in F.delta], F.least, F.decided))
    print("\n".join(lines))
    for (name, reg), F in census.items():
        assert F.decided and F.n_untestable == 0 and len(F.pairs) == 8, (name, reg)
        exp = js.EXPECT[name]
        if exp is not None:
            assert F.kept == exp[0], (name, reg, F.kept)
            assert exp[1] is None or F.order == exp[1], (name, reg, F.order)
        assert not F.kept or F.J < F.gate[len(F.kept)]
    for reg in js.REGIMES:
        F = census[("common", reg)]
        assert F.rounds == 1 and 0.8 < F.delta[0] < 1.0 and abs(F.delta[1]) < 0.05 and abs(F.delta[2]) < 0.01      # the shift, shrunk by the prior
        F = census[("alternating", reg)]
        assert len(F.order) >= 2 and all(a % 2 == 1 for a in F.order), (reg, F.order)                              # the minority sign leaves
        assert census[("outliers2", reg)].rounds == 3 and census[("hopeless", reg)].rounds == 9
        F = census[("nocov", reg)]
        assert F.delta == [0, 0, 0] and F.J == sum(F.pairs[a].t[0].v for a in range(8))


def test_the_checker_has_teeth(census):
    """the reference's own result passes; a kept pair that should have left, a J off by 3 B, a J of another kept set, a wrong count and a cone
    that is not the hypothesis' are each rejected"""
    for (name, reg), F in census.items():
        idx = F.expect_index(); J = float(F.J); dl = [float(d) for d in F.delta]; nk, nd = len(F.kept), len(F.order)
        assert not F.failures(idx, J, nk, nd, 0, dl), (name, reg, F.failures(idx, J, nk, nd, 0, dl))
        assert F.failures(idx, J + 3 * float(F.B) + 1e-300, nk, nd, 0, dl) if F.kept else True
        assert F.failures(idx, J, nk + 1, nd, 0, dl) and F.failures(idx, J, nk, nd, 1, dl)
        if F.order:
            back = list(idx); back[F.order[-1]] = F.hyp[F.order[-1]]
            assert F.failures(back, J, nk + 1, nd - 1, 0, dl), (name, reg)
            Jb = float(F.J_of(sorted(F.kept + [F.order[-1]]))[0])
            assert any("gate" in w or "reference" in w for w in F.failures(back, Jb, nk + 1, nd - 1, 0, dl)), (name, reg)
        if F.kept:
            wrong = list(idx); wrong[F.kept[0]] = (idx[F.kept[0]] + 1) % 8
            assert any("hypothesis" in w for w in F.failures(wrong, J, nk, nd, 0, dl))
