"""CPU tests of the covariance-gated association: what the cases of assoc_nn_shapes.py reach (a census, from the exact reference alone), that
the checker of assoc_nn_ref.py has teeth, that at most 1 % of a case's queries are ambiguous, and the C-ABI's host-side refusals on a
host-only handle.  nn_numpy below is the header's formula in numpy fp64, operation by operation — an answer for the checker to check where
there is no device; it proves nothing about the kernels."""
import ctypes as C

import numpy as np
import pytest

import assoc_exec as ax
import assoc_nn_ref as nr
import assoc_nn_shapes as ns

NEW_FUNCS = ("gs_nn_params_default", "gs_map_set_cov", "gs_map_get_cov", "gs_map_set_cov_from_marginals", "gs_associate_nn_batch",
             "gs_associate_nn_resident", "gs_frame_frontend_nn", "gs_debug_time_associate_nn_resident")


def nn_numpy(c, gxy=None, params=None, pose_cov="case", map_xy=None, map_ty=None, map_cov="case"):
    """(idx, d2, second, info) of a case by the header's formula in fp64; info: per query the Euclidean-nearest type-matching cone within
    max_distance (-1: none) and whether some type-matching cone beyond max_distance lies inside the gate"""
    p = nr.params_of(**(c["params"] if params is None else params))
    poses, pose_of, ob = c["poses"], c["pose_of"], c["obs"]
    map_xy = c["map_xy"] if map_xy is None else map_xy; map_ty = c["map_ty"] if map_ty is None else map_ty
    map_cov = c["map_cov"] if isinstance(map_cov, str) else map_cov; pose_cov = c["pose_cov"] if isinstance(pose_cov, str) else pose_cov
    m = len(map_xy); cov = np.zeros((m, 4)) if map_cov is None else np.asarray(map_cov).reshape(-1, 4)
    n = len(ob); idx = np.full(n, -1, dtype=np.int32); d2o = np.full(n, np.inf); sec = np.full(n, np.inf)
    nearest = np.full(n, -1); beyond = np.zeros(n, dtype=bool)
    z = ax.polar_to_xy(ob[:, 0], ob[:, 1], ob[:, 2], c["lidar"])
    with np.errstate(all="ignore"):
        for i in range(n):
            t = poses[pose_of[i]]; cs, sn = np.cos(t[2]), np.sin(t[2]); zx, zy = z[i]
            wx, wy = zx * cs - zy * sn, zx * sn + zy * cs
            gx, gy = (wx + t[0], wy + t[1]) if gxy is None else gxy[i]
            r2 = zx * zx + zy * zy
            if not (np.isfinite(gx) and np.isfinite(gy) and r2 > 0) or m == 0:
                continue
            k = (p["sigma_range"] * p["sigma_range"]) / r2; sb2 = p["sigma_bearing"] * p["sigma_bearing"]; sx2 = p["sigma_xy"] * p["sigma_xy"]
            a00 = ((k * wx) * wx + (sb2 * wy) * wy) + sx2; a01 = (k * wx) * wy - (sb2 * wx) * wy; a11 = ((k * wy) * wy + (sb2 * wx) * wx) + sx2
            if pose_cov is not None:
                pc = np.asarray(pose_cov).reshape(-1, 9)[pose_of[i]]; ux, uy = -wy, wx
                a00 = a00 + ((pc[0] + (2.0 * pc[2]) * ux) + (pc[8] * ux) * ux)
                a01 = a01 + (((pc[1] + pc[2] * uy) + pc[5] * ux) + (pc[8] * ux) * uy)
                a11 = a11 + ((pc[4] + (2.0 * pc[5]) * uy) + (pc[8] * uy) * uy)
            n0, n1 = map_xy[:, 0] - gx, map_xy[:, 1] - gy
            eu = np.sqrt(n0 * n0 + n1 * n1)
            s00, s01, s11 = cov[:, 0] + a00, cov[:, 1] + a01, cov[:, 3] + a11
            det = s00 * s11 - s01 * s01
            d2 = (((s11 * n0) * n0 - ((2.0 * s01) * n0) * n1) + (s00 * n1) * n1) / det
            ty = np.abs(map_ty.astype(np.float64) - ob[i, 3]) < p["type_tol"]
            gate = ty & (det > 0) & (s00 > 0) & (d2 < p["gate_chi2"])
            ok = gate & (eu < p["max_distance"])
            beyond[i] = (gate & ~(eu < p["max_distance"])).any()
            te = np.where(ty & (eu < p["max_distance"]), eu, np.inf)
            nearest[i] = int(te.argmin()) if np.isfinite(te).any() else -1
            if ok.any():
                v = np.where(ok, d2, np.inf); j = int(v.argmin()); idx[i] = j; d2o[i] = v[j]
                v[j] = np.inf; sec[i] = v.min()
    return idx, d2o, sec, dict(nearest=nearest, beyond=beyond)


@pytest.fixture(scope="module")
def answers():
    """nn_numpy of every case, computed once"""
    return {name: nn_numpy(ns.case(name)) for name in ns.NAMES}


@pytest.mark.parametrize("name", ns.NAMES)
def test_the_numpy_formula_is_admissible_and_few_queries_are_ambiguous(name, answers):
    c = ns.case(name); R = ns.reference(name); idx, d2, sec, _ = answers[name]
    w = R.check(idx, d2, sec, name)
    amb = R.n_ambiguous()
    print("%-16s n %3d map %4d exact pairs %5d ambiguous %d worst d2 %.3f second %.3f" % (name, len(idx), len(c["map_xy"]), R.n_pairs, amb, w[0], w[1]))
    assert not c["tie"]
    assert amb <= 0.01 * len(idx), (name, amb, len(idx))                   # the cap, from the reference alone
    u = R.unique_answer()
    for i, j in c["notes"].get("expect", {}).items():
        assert u[i] == j and idx[i] == j, (name, i, int(u[i]), int(idx[i]), j)
    for i, j in c["notes"].get("expect_cone", {}).items():
        assert u[i] in (j, -1), (name, i, int(u[i]), j)


def test_census_every_outcome_is_reached(answers):
    seen = {k: [] for k in ("match", "none", "nan_query", "runner_up", "no_runner_up", "not_the_euclidean_nearest", "in_gate_beyond_max_distance",
                            "type_mismatch_on_the_nearest", "elongated_beats_nearer", "heading_variance_admits", "indefinite_skipped", "zero_diagonal_indefinite_skipped",
                            "det_zero", "no_map_cov", "no_pose_cov", "second_tile", "grid_size", "candidate_outside_the_gate", "two_cells_one_bucket")}
    for name in ns.NAMES:
        c = ns.case(name); R = ns.reference(name); idx, d2, sec, info = answers[name]; u = R.unique_answer()
        def mark(k, cond):
            if cond:
                seen[k].append(name)
        mark("match", (u >= 0).any()); mark("none", ((u == -1) & R.valid).any()); mark("nan_query", (~R.valid).any())
        mark("runner_up", np.isfinite(sec).any()); mark("no_runner_up", ((idx >= 0) & np.isinf(sec)).any())
        mark("not_the_euclidean_nearest", ((u >= 0) & (u != info["nearest"])).any()); mark("in_gate_beyond_max_distance", info["beyond"].any())
        mark("no_map_cov", c["map_cov"] is None); mark("no_pose_cov", c["pose_cov"] is None)
        mark("second_tile", (u >= 1024).any()); mark("grid_size", len(c["map_xy"]) >= 2048)
        mark("candidate_outside_the_gate", any(cd.d2 is not None and not cd.poss for cs in R.cands for cd in cs))
        mark("det_zero", any(cd.det == 0 for cs in R.cands for cd in cs)); mark("indefinite_skipped", any(cd.det < 0 for cs in R.cands for cd in cs))
    c = ns.case("type_mismatch"); mark = lambda k: seen[k].append("planted")
    assert answers["type_mismatch"][0][0] == 9 and c["map_ty"][5] != c["obs"][0, 3]; mark("type_mismatch_on_the_nearest")
    c = ns.case("elongated"); g = c["gxy"][0]
    assert answers["elongated"][0][0] == 8 and np.hypot(*(c["map_xy"][4] - g)) < np.hypot(*(c["map_xy"][8] - g)); mark("elongated_beats_nearer")
    assert answers["elongated"][3]["nearest"][0] == 4
    c = ns.case("grid_twice"); u = ns.reference("grid_twice").unique_answer()
    for i in c["notes"]["alone"]:
        bk = ns.nine_buckets(c["gxy"][i], len(c["map_xy"])); own = ns.nine_buckets(c["map_xy"][10 + i], len(c["map_xy"]))[4]
        assert bk.count(own) == 2 and u[i] == 10 + i and np.isinf(answers["grid_twice"][2][i]), (i, bk, own, int(u[i]))
    mark("two_cells_one_bucket")
    Rw = ns.reference_without_pose_cov("heading")
    assert ns.reference("heading").unique_answer().tolist() == [10, 11] and Rw.unique_answer().tolist() == [-1, -1]; mark("heading_variance_admits")
    assert ns.reference("indefinite").unique_answer()[1] == -1; mark("zero_diagonal_indefinite_skipped")
    print("\n".join("%-30s %s" % (k, " ".join(v)) for k, v in seen.items()))
    missing = [k for k, v in seen.items() if not v]
    assert not missing, missing


def test_exact_by_construction_cases_in_numpy():
    """the gate, the distance and the tie cases on numpy's own global XY: the expectations of assoc_nn_shapes.exact_cases hold for the formula in fp64"""
    base = dict(lidar=ns.LIDAR, poses=ns.EQ_POSE, pose_of=np.zeros(len(ns.EQ_OBS), dtype=np.int32), obs=ns.EQ_OBS, pose_cov=None, params={})
    g = ax.cone_to_global(ns.EQ_POSE, base["pose_of"], ns.EQ_OBS, ns.LIDAR); n = 0
    for kind, i, xy, ty, cov, prm, ej, ed, es in ns.exact_cases(g):
        idx, d2, sec, _ = nn_numpy(base, gxy=g, params=prm, pose_cov=None, map_xy=xy, map_ty=ty, map_cov=cov)
        assert idx[i] == ej and d2[i] == ed and sec[i] == es, (kind, i, int(idx[i]), ej, d2[i], ed, sec[i], es)
        n += 1
    assert n == 4 * 2 * 5


def test_the_checker_has_teeth(answers):
    """a swapped index, a d2 off by 3 B and second_d2 replaced by d2 are each rejected"""
    name = "random2048"; R = ns.reference(name); idx, d2, sec, _ = answers[name]; u = R.unique_answer()
    assert not R.failures(idx, d2, sec)
    multi = [i for i in range(len(idx)) if u[i] >= 0 and np.isfinite(sec[i])]
    assert len(multi) >= 10
    for i in multi[:10]:
        other = [cd for cd in R.cands[i] if cd.sure and cd.j != idx[i]][0]
        a = idx.copy(); a[i] = other.j
        assert [q for q, _ in R.failures(a, d2, sec)] == [i], "a swapped index"
        a = d2.copy(); a[i] = float(d2[i] + 3 * float(R.win[i][0].B))
        assert [q for q, _ in R.failures(idx, a, sec)] == [i], "d2 off by 3 B"
        a = sec.copy(); a[i] = d2[i]
        assert [q for q, _ in R.failures(idx, d2, a)] == [i], "second_d2 replaced by d2"
    i = int(np.flatnonzero(u >= 0)[0]); a = idx.copy(); a[i] = -1; b = d2.copy(); b[i] = np.inf; s = sec.copy(); s[i] = np.inf
    assert [q for q, _ in R.failures(a, b, s)] == [i], "-1 where a cone is surely admissible"
    i = int(np.flatnonzero(u == -1)[0]); a = idx.copy(); a[i] = 0
    assert [q for q, _ in R.failures(a, d2, sec)] == [i], "a cone where none is admissible"


def test_the_header_declares_and_the_library_exports(pkg):
    names = pkg.binding.declared_symbols(); L = pkg.binding.lib()
    for f in NEW_FUNCS:
        assert f in names, f
        assert hasattr(L, f), f


def test_defaults_and_refusals_on_a_host_only_handle(pkg):
    b = pkg.binding; L = b.lib()
    p = b.NnParams(); assert L.gs_nn_params_default(C.byref(p)) == 0 and L.gs_nn_params_default(None) == -1
    assert p.struct_size == C.sizeof(b.NnParams) == 56 and p.reserved == 0
    assert {k: getattr(p, k) for k in nr.DEFAULTS} == nr.DEFAULTS
    G = pkg.Graph(device=-2)
    poses = np.zeros((1, 3)); po = np.zeros(2, dtype=np.int32); ob = np.array([[10.0, 0, 5, 1], [20.0, 0, 6, 2]]); xy = np.ones((3, 2)); ty = np.ones(3, dtype=np.int32)
    def code(fn, *a, **kw):
        with pytest.raises(b.GsError) as e:
            fn(*a, **kw)
        return e.value.code
    bad = [dict(gate_chi2=0.0), dict(gate_chi2=-1.0), dict(max_distance=0.0), dict(max_distance=-3.0), dict(sigma_range=-1e-9), dict(sigma_bearing=-1.0),
           dict(sigma_xy=-0.05), dict(struct_size=48), dict(struct_size=0)]
    bad += [{k: v} for k in nr.DEFAULTS for v in (float("nan"), float("inf"), -float("inf"))]
    da = C.c_void_p(4096)                                                # never dereferenced: every refusal below is decided on the host
    for kw in bad:
        prm = b.nn_params(**kw)
        assert code(G.associate_nn, poses, po, ob, xy, ty, params=prm) == -1, kw
        assert code(G.frame_frontend_nn, poses[0], ob, params=prm) == -1, kw
        assert L.gs_associate_nn_resident(G.h, 2, da, 1, da, da, None, C.byref(prm), da, None, None) == -1, kw
    prm = b.nn_params()
    assert code(G.associate_nn, poses, po, ob, xy, ty) == -4 and code(G.frame_frontend_nn, poses[0], ob) == -4           # good arguments: GS_ERR_NO_DEVICE
    assert L.gs_associate_nn_resident(G.h, 2, da, 1, da, da, None, C.byref(prm), da, None, None) == -4
    assert L.gs_associate_nn_resident(G.h, 2, da, 1, da, C.c_void_p(4096 + 8), None, C.byref(prm), da, None, None) == -1  # dev_obs not 32-byte aligned
    assert L.gs_associate_nn_resident(G.h, 2, da, 1, da, da, None, None, da, None, None) == -1                           # null params
    assert L.gs_associate_nn_resident(G.h, 2, None, 1, da, da, None, C.byref(prm), da, None, None) == -1
    assert L.gs_associate_nn_resident(None, 2, da, 1, da, da, None, C.byref(prm), da, None, None) == -1
    assert code(G.associate_nn, poses, np.array([0, 1], dtype=np.int32), ob, xy, ty) == -1                                # pose_of_obs out of range (batch: refused)
    dp = C.POINTER(C.c_double); ip = C.POINTER(C.c_int32); out = np.zeros(2, dtype=np.int32)
    args = lambda **kw: [kw.get(k, v) for k, v in (("g", G.h), ("n", 2), ("poses", poses.ctypes.data_as(dp)), ("np", 1), ("po", po.ctypes.data_as(ip)),
                                                   ("ob", ob.ctypes.data_as(dp)), ("m", 3), ("xy", xy.ctypes.data_as(dp)), ("ty", ty.ctypes.data_as(ip)), ("mc", None), ("pc", None),
                                                   ("prm", C.byref(prm)), ("out", out.ctypes.data_as(ip)), ("d2", None), ("sec", None))]
    assert L.gs_associate_nn_batch(*args()) == -4
    for k in ("g", "poses", "po", "ob", "xy", "ty", "prm", "out"):
        assert L.gs_associate_nn_batch(*args(**{k: None})) == -1, k
    assert L.gs_associate_nn_batch(*args(n=-1)) == -1 and L.gs_associate_nn_batch(*args(m=-1)) == -1
    z = np.zeros(4); i2 = np.zeros(2, dtype=np.int32)
    fa = lambda **kw: [kw.get(k, v) for k, v in (("g", G.h), ("pose", poses.ctypes.data_as(dp)), ("pc", None), ("ob", ob.ctypes.data_as(dp)), ("k", 2), ("prm", C.byref(prm)),
                                                 ("z", z.ctypes.data_as(dp)), ("gx", z.ctypes.data_as(dp)), ("i", i2.ctypes.data_as(ip)), ("d2", z.ctypes.data_as(dp)), ("s", z.ctypes.data_as(dp)))]
    assert L.gs_frame_frontend_nn(*fa()) == -4
    for k in ("g", "pose", "ob", "prm", "z", "gx", "i", "d2", "s"):
        assert L.gs_frame_frontend_nn(*fa(**{k: None})) == -1, k
    # the map's covariances: an empty map, so every range is beyond its end; malformed blocks are refused before that matters
    assert G.map_size() == 0
    assert code(G.map_set_cov, 0, [[1, 0, 0, 1]]) == -1 and code(G.map_cov, 0, 1) == -1 and code(G.map_set_cov_from_marginals, 0, [3]) == -1
    assert L.gs_map_set_cov(G.h, 0, 1, None) == -1 and L.gs_map_get_cov(G.h, 0, 1, None) == -1 and L.gs_map_set_cov_from_marginals(G.h, 0, 1, None) == -1
    assert L.gs_map_set_cov(G.h, -1, 0, None) == -1 and L.gs_map_set_cov(G.h, 0, -1, None) == -1
    assert L.gs_map_set_cov(G.h, 0, 0, None) == -4                                    # nothing to refuse: the device is asked for
    G.close()
