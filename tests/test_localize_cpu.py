"""CPU tests of frame localisation: the header declares and the library exports it, gs_loc_params_default, every host-side refusal on a
host-only handle, the exact reference (localize_ref.py) against a dense minimisation in measurement space, the census of the purpose-made scenes
(localize_shapes.py: every frame DECIDED by the reference alone, each doing what it was made for), and the teeth of the two checkers.
Nothing here runs a kernel."""
import ctypes as C

import numpy as np
import pytest

import localize_ref as lr
import localize_shapes as ls

NEW_FUNCS = ("gs_loc_params_default", "gs_localize_batch", "gs_localize_resident", "gs_frame_frontend_localize", "gs_debug_localize",
             "gs_debug_time_localize_resident")
mpf = lr.mpf


def test_the_header_declares_and_the_library_exports(pkg):
    names = pkg.binding.declared_symbols(); L = pkg.binding.lib()
    for f in NEW_FUNCS:
        assert f in names, f
        assert hasattr(L, f), f
    for f in ("localize", "localize_resident", "frame_frontend_localize", "time_localize_resident", "debug_localize"):
        assert hasattr(pkg.Graph, f), f


def test_the_default_params(pkg):
    b = pkg.binding; p = b.loc_params()
    assert C.sizeof(b.LocParams) == 24 and p.struct_size == 24
    assert (p.max_iterations, p.tol_xy, p.tol_theta) == (5, 1e-6, 1e-8) and b.LOC_ITER_MAX == 16
    assert b.lib().gs_loc_params_default(None) == -1
    assert b.loc_params(max_iterations=3, tol_xy=0.0).max_iterations == 3
    with pytest.raises(AttributeError):
        b.loc_params(nothing=1)


def test_refusals_on_a_host_only_handle(pkg):
    b = pkg.binding; L = b.lib(); G = pkg.Graph(device=-2)
    poses = np.zeros((2, 3)); po = np.zeros(2, dtype=np.int32); ob = np.array([[10.0, 0, 5, 1], [20.0, 0, 6, 2]]); xy = np.ones((3, 2))
    fs = np.array([0, 1, 2], dtype=np.int32); hyp = np.array([2, -1], dtype=np.int32)
    def code(fn, *a, **kw):
        with pytest.raises(b.GsError) as e:
            fn(*a, **kw)
        return e.value.code
    da = C.c_void_p(4096)                                                    # never dereferenced: every refusal below is decided on the host
    prm = b.nn_params(); jc = b.jc_params(); loc = b.loc_params()
    res = lambda **kw: L.gs_localize_resident(*[kw.get(k, v) for k, v in (("g", G.h), ("n", 2), ("p", da), ("np", 1), ("po", da), ("ob", da), ("nf", 2), ("fs", da),
                                                                            ("pc", None), ("prm", C.byref(prm)), ("loc", C.byref(loc)), ("in", da), ("pose", None),
                                                                            ("cov", None), ("chi2", None), ("pairs", None), ("it", None), ("st", None))])
    # good arguments: GS_ERR_NO_DEVICE; every output is optional
    assert code(G.localize, poses, po, ob, fs, xy, hyp) == -4 and code(G.frame_frontend_localize, poses[0], ob) == -4
    assert code(G.localize, poses, po, ob, [0, 0, 2, 2], xy, hyp) == -4                                                       # empty frames are allowed
    assert res() == -4 and res(pose=da, cov=da, chi2=da, pairs=da, it=da, st=da, pc=da) == -4
    # gs_loc_params
    bad = [dict(struct_size=0), dict(struct_size=32), dict(max_iterations=0), dict(max_iterations=17), dict(max_iterations=-1)]
    bad += [{k: v} for k in ("tol_xy", "tol_theta") for v in (-1e-30, float("nan"), float("inf"), -float("inf"))]
    for kw in bad:
        l = b.loc_params()
        for k, v in kw.items():
            setattr(l, k, v)
        assert code(G.localize, poses, po, ob, fs, xy, hyp, loc=l) == -1, kw
        assert code(G.frame_frontend_localize, poses[0], ob, loc=l) == -1, kw
        assert res(loc=C.byref(l)) == -1, kw
    for kw in (dict(max_iterations=1), dict(max_iterations=16), dict(tol_xy=0.0, tol_theta=0.0)):
        assert code(G.localize, poses, po, ob, fs, xy, hyp, loc=b.loc_params(**kw)) == -4, kw
    # the sigmas and struct_size of gs_nn_params; the other fields are read by the frame call's assignment only
    bad = [dict(sigma_range=-1e-9), dict(sigma_bearing=-1.0), dict(sigma_xy=-0.05), dict(struct_size=48), dict(struct_size=0)]
    bad += [{k: v} for k in ("sigma_range", "sigma_bearing", "sigma_xy") for v in (float("nan"), float("inf"))]
    for kw in bad:
        p = b.nn_params(**kw)
        assert code(G.localize, poses, po, ob, fs, xy, hyp, params=p) == -1, kw
        assert code(G.frame_frontend_localize, poses[0], ob, params=p) == -1, kw
        assert res(prm=C.byref(p)) == -1, kw
    for kw in (dict(gate_chi2=-1.0), dict(max_distance=0.0)):
        p = b.nn_params(**kw)
        assert code(G.localize, poses, po, ob, fs, xy, hyp, params=p) == -4 and res(prm=C.byref(p)) == -4, kw
        assert code(G.frame_frontend_localize, poses[0], ob, params=p) == -1, kw
    t = b.jc_params(); t.gate[3] = -0.5                                                                                       # the frame call reads the table
    assert code(G.frame_frontend_localize, poses[0], ob, jc=t) == -1
    # pointers, counts, alignment (resident)
    assert res(ob=C.c_void_p(4096 + 8)) == -1
    for k in ("g", "p", "po", "ob", "fs", "prm", "loc", "in"):
        assert res(**{k: None}) == -1, k
    assert res(n=-1) == -1 and res(nf=-1) == -1 and res(np=-1) == -1
    # the hypothesis, the pose indices, the frames (batch)
    for h in ([3, -1], [-2, 0], [0, 2 ** 30]):
        assert code(G.localize, poses, po, ob, fs, xy, h) == -1, h
    assert code(G.localize, poses, np.array([0, 2], dtype=np.int32), ob, fs, xy, hyp) == -1
    assert code(G.localize, poses, np.array([0, 1], dtype=np.int32), ob, [0, 2], xy, hyp) == -1                               # a frame with two poses
    assert code(G.localize, poses, np.array([0, 1], dtype=np.int32), ob, fs, xy, hyp) == -4
    for f in ([1, 1, 2], [0, 2, 1, 2], [0, 1, 1], [0, 1, 3], [0, 2, 1]):
        assert code(G.localize, poses, po, ob, f, xy, hyp) == -1, f
    big = np.tile(ob[:1], (300, 1)); pob = np.zeros(300, dtype=np.int32); hb = np.full(300, -1, dtype=np.int32)
    assert code(G.localize, poses, pob, big, [0, 257, 300], xy, hb) == -1 and code(G.localize, poses, pob, big, [0, 44, 300], xy, hb) == -4
    assert code(G.frame_frontend_localize, poses[0], big[:257]) == -1 and code(G.frame_frontend_localize, poses[0], big[:256]) == -4
    dp = C.POINTER(C.c_double); ip = C.POINTER(C.c_int32)
    args = lambda **kw: [kw.get(k, v) for k, v in (("g", G.h), ("n", 2), ("poses", poses.ctypes.data_as(dp)), ("np", 2), ("po", po.ctypes.data_as(ip)),
                                                   ("ob", ob.ctypes.data_as(dp)), ("nf", 2), ("fs", fs.ctypes.data_as(ip)), ("m", 3), ("xy", xy.ctypes.data_as(dp)),
                                                   ("mc", None), ("pc", None), ("prm", C.byref(prm)), ("loc", C.byref(loc)), ("in", hyp.ctypes.data_as(ip)),
                                                   ("pose", None), ("cov", None), ("chi2", None), ("pairs", None), ("it", None), ("st", None))]
    assert L.gs_localize_batch(*args()) == -4
    for k in ("g", "poses", "po", "ob", "fs", "xy", "prm", "loc", "in"):
        assert L.gs_localize_batch(*args(**{k: None})) == -1, k
    assert L.gs_localize_batch(*args(n=-1)) == -1 and L.gs_localize_batch(*args(m=-1)) == -1 and L.gs_localize_batch(*args(nf=-1)) == -1
    assert L.gs_debug_localize(G.h, 2, None) == -1 and L.gs_debug_localize(G.h, -2, None) == -1 and L.gs_debug_localize(None, 0, None) == -1
    assert L.gs_debug_localize(G.h, 1, None) == 0 and L.gs_debug_localize(G.h, -1, None) == 0
    ms = C.c_double()
    tm = lambda reps: L.gs_debug_time_localize_resident(G.h, 2, da, 1, da, da, 2, da, None, C.byref(prm), C.byref(loc), da, None, None, None, None, None, None, reps, C.byref(ms))
    assert tm(0) == -1 and tm(3) == -4
    G.close()


@pytest.fixture(scope="module")
def census():
    """scene -> (Frame, its exact run)"""
    out = {}
    for name in ls.NAMES:
        c = ls.scene(name); F = lr.make(c, c["hyp"], c["frame_start"])[0]
        out[name] = (F, F.run(**dict(dict(max_iterations=5, tol_xy=1e-6, tol_theta=1e-8), **c["loc"])))
    return out


def test_census_every_scene_is_decided_and_does_what_it_was_made_for(census):
    lines = []
    for name, (F, r) in census.items():
        lines.append("%-15s status %d iterations %d pairs %d d (%.9g, %.9g, %.9g) chi2 %.9g B pose (%.3g, %.3g, %.3g) B cov00 %.3g B chi2 %.3g least margin %.3g B decided %d" % (
            name, r.status, r.iterations, r.n_pairs, *[float(t.v) for t in r.d], float(r.chi2.v), *[float(2 * t.e) for t in r.pose], float(2 * r.cov[0].e),
            float(2 * r.chi2.e), r.least, r.decided))
    print("\n".join(lines))
    for name, (F, r) in census.items():
        c = ls.scene(name)
        assert r.decided, name
        if c["expect"] is not None:
            assert (r.status, r.iterations) == c["expect"], (name, r.status, r.iterations)
    r = census["shift"][1]
    assert abs(r.d[0].v + mpf(3) / 8) < 1e-12 and abs(r.chi2.v - mpf(3) / 16) < 1e-12 and abs(r.cov[0].v - mpf(1) / 4) < 1e-12 and r.cov[8].v == 0 and r.n_pairs == 3
    # the rotation: one linear step stays far from the converged pose — more than 1000 B, and centimetres
    one, full = census["rotation_one"][1], census["rotation"][1]
    assert full.status == 0 and 2 <= full.iterations <= 5 and census["rotation_limit"][1].status == 1
    for t in range(3):
        assert abs(one.pose[t].v - full.pose[t].v) > 1000 * 2 * (one.pose[t].e + full.pose[t].e), t
    assert abs(one.pose[0].v - full.pose[0].v) > 4e-3 and abs(one.pose[2].v - full.pose[2].v) > 1e-4 and abs(full.pose[2].v - mpf(0.1)) < 5e-4
    assert one.chi2.v > full.chi2.v + 1e-3
    # the wide prior: the answer is the truth to within the cones' own residual, and B says how many digits the Woodbury form keeps
    F, r = census["wide"]
    assert r.status == 0 and all(abs(r.pose[t].v - mpf(float(ls.scene("wide")["truth"][t]))) < 1e-6 for t in range(3))
    print("wide prior: B of the pose (%.3g, %.3g, %.3g), of cov00 %.3g (relative %.3g)" % (*[float(2 * t.e) for t in r.pose], float(2 * r.cov[0].e),
                                                                                       float(2 * r.cov[0].e / abs(r.cov[0].v))))
    assert all(2 * t.e < 1e-9 for t in r.pose)
    F, r = census["singular"]
    assert r.status == 0 and r.pose[1].v == mpf(-2) and r.pose[2].v == 0 and r.cov[4].v == 0 and r.cov[8].v == 0 and abs(r.d[0].v - mpf(8) / 18) < 1e-9
    F, r = census["nocov"]
    assert r.iterations == 0 and all(t.v == 0 for t in r.cov) and r.chi2.v > 0 and r.n_pairs == 8
    F, r = census["none"]
    assert r.n_pairs == 0 and r.chi2.v == 0 and [t.v for t in r.pose] == [3, -2, 0] and r.cov[0].v == 1
    assert census["one"][1].n_pairs == 1 and census["two"][1].n_pairs == 2 and census["one"][1].status == 0 and census["two"][1].status == 0
    assert census["nonfinite"][1].n_pairs == 7 and census["nanquery"][1].n_pairs == 7 and census["nonfinite"][1].status == 0
    print("least margin over the scenes: %.3g B" % min(r.least for _, r in census.values()))


def test_the_reference_against_the_dense_minimisation(census):
    """where the iteration converged, its pose is the fixed point of the dense measurement-space iteration to within the tolerance, the exact
    step there is below the tolerance, and its covariance is the dense one at its own pose"""
    for name, (F, r) in census.items():
        if F.P is None or r.status != 0 or r.iterations == 0:
            continue
        x, steps = F.minimise()
        tols = (1e-6, 1e-6, 1e-8)
        for t in range(3):
            assert abs(r.pose[t].v - x[t]) <= tols[t], (name, t, float(r.pose[t].v - x[t]))
        st = F.step_at_mp([t.v for t in r.pose])
        assert all(abs(st[t]) <= tols[t] for t in range(3)), (name, [float(t) for t in st])
        pf = [float(t.v) for t in r.pose]; cv = F.cov_at(pf); cm = F.cov_meas_at(pf); sa = F.step_at(pf); sm = F.step_at_mp([mpf(t) for t in pf])
        assert all(abs(cv[t] - cm[t]) <= mpf(10) ** -40 * max(1, abs(cm[t])) for t in range(9)), name     # the checkers' 3 x 3 form against measurement space
        assert all(abs(sa[t] - sm[t]) <= mpf(10) ** -40 for t in range(3)), name
        for t in range(9):
            assert abs(cv[t] - r.cov[t].v) <= 1e-12 * max(1, abs(cv[t])) + 2 * r.cov[t].e, (name, t)
        print("%-10s dense iteration: %d steps, |pose - fixed point| (%.3g, %.3g, %.3g)" % (name, steps, *[float(abs(r.pose[t].v - x[t])) for t in range(3)]))


def test_the_checkers_have_teeth(census):
    """the reference's own result passes; a pose off by more than the tolerance, a covariance entry off by 3 B, a chi2 off by 3 B and a wrong
    count are each rejected"""
    for name, (F, r) in census.items():
        c = ls.scene(name); kw = dict(dict(max_iterations=5, tol_xy=1e-6, tol_theta=1e-8), **c["loc"])
        pose = [float(t.v) for t in r.pose]; cov = [float(t.v) for t in r.cov]; chi2 = float(r.chi2.v)
        good = (pose, cov, chi2, r.n_pairs, r.iterations, r.status)
        assert not F.failures(good, **kw), (name, F.failures(good, **kw))
        assert F.failures((pose, cov, chi2, r.n_pairs, r.iterations, 1 - r.status if r.status < 2 else 0), **kw), name
        assert F.failures((pose, cov, chi2, r.n_pairs + 1, r.iterations, r.status), **kw), name
        if r.status == 0 and r.iterations > 0:
            moved = list(pose); moved[0] += 1e-5
            assert any("step" in w for w in F.failures((moved, cov, chi2, r.n_pairs, r.iterations, r.status), **kw)), name
            worse = list(cov); worse[0] += 3 * float(2 * r.cov[0].e) + 1e-300
            assert any("dense" in w for w in F.failures((pose, worse, chi2, r.n_pairs, r.iterations, r.status), **kw)), name
        if r.status != 2:
            assert any("chi2" in w for w in F.failures((pose, cov, chi2 + 3 * float(2 * r.chi2.e) + 1e-300, r.n_pairs, r.iterations, r.status), **kw)), name
