"""GPU tests of the covariance-gated association (gs_assoc_nn.hip) against the exact reference of tests/assoc_nn_ref.py, on every path and every
case of tests/assoc_nn_shapes.py (test_assoc_nn_cpu.py holds the census of what each case reaches and shows that the checker has teeth).

Every case runs through gs_associate_nn_batch with assoc_grid 0, 1 and -1 and gs_associate_nn_resident with the grid and with brute force:
the five results must agree BIT FOR BIT in index, d2 and second_d2, and each is held to the checker (the index an admissible winner, d2
within its bound B of that cone's exact value, second_d2 within its bound of an admissible runner-up's).  gs_frame_frontend_nn, pose by pose, is
held to the same checker and must return the same bits; its z and g are held to frontend_exact_ref's bounds.  Equality with the gate and with
max_distance, and an exact tie, are asserted bit for bit from the frame path's OWN reported global XY (assoc_nn_shapes.exact_cases); the
resident covariances are followed through append / set / clear / growth / partial and refused sets, and taken from the marginals.

Measured on an MI355X (profiles/assoc_nn_gpu_suite.txt has every case), worst |got - exact| / B of d2 / second_d2 per kernel and case
family, and of the frame kernel's z / g against frontend_exact_ref's bounds; the bound comes from the rounding count in assoc_nn_ref's
docstring alone and was not fitted to these:
  family    k_assoc_nn       k_assoc_nn_grid   k_frame_nn        k_frame_nn z / g
  shape     0.040 / 0.035    0.040 / 0.035     0.040 / 0.035     0.212 / 0.102
  grid      0.176 / 0.022    0.176 / 0.022     0.176 / 0.022     0.180 / 0.230
  cov       0.009 / 0.000    0.009 / 0.000     0.009 / 0.000     0.210 / 0.077
  random    0.037 / 0.026    0.037 / 0.026     0.037 / 0.026     0.231 / 0.107
The three kernels' columns are equal because their outputs are: on all 25 cases the five batch / resident results and the frame path agreed
bit for bit in index, d2 and second_d2, and every unambiguous query returned the reference's winner.  The 40 exact-by-construction cases
(gate, max_distance, tie) held bit for bit on all six paths.
"""
import ctypes as C

import numpy as np
import pytest

import assoc_nn_ref as nr
import assoc_nn_shapes as ns
import frontend_exact_ref as fx

pytestmark = pytest.mark.gpu
STATS = {}


@pytest.fixture(scope="module")
def G(pkg):
    if pkg.device_count() < 1:
        pytest.fail("no gfx950 device visible: the HIP path cannot run")
    g = pkg.Graph(lidar_to_cog=ns.LIDAR)
    yield g
    g.close()


class Dev:
    """a case's poses, pose indices, observations and pose covariances in device memory, with result buffers"""

    def __init__(self, pkg, poses, pose_of, obs, pose_cov=None):
        DA = pkg.binding.DeviceArray; f = lambda a, t: DA(np.ascontiguousarray(a, dtype=t))
        self.n = len(obs); self.np = len(poses)
        self.p, self.po, self.ob = f(poses, np.float64), f(pose_of, np.int32), f(obs, np.float64)
        self.pc = None if pose_cov is None else f(pose_cov, np.float64)
        self.idx, self.d2, self.sec = DA(nbytes=4 * self.n), DA(nbytes=8 * self.n), DA(nbytes=8 * self.n)

    def resident(self, G, params):
        G.associate_nn_resident(self.p, self.np, self.po, self.ob, self.n, self.idx, self.d2, self.sec, self.pc, params); G.synchronize()
        return self.idx.to_host(np.int32, self.n), self.d2.to_host(np.float64, self.n), self.sec.to_host(np.float64, self.n)

    def free(self):
        for a in (self.p, self.po, self.ob, self.pc, self.idx, self.d2, self.sec):
            if a is not None:
                a.free()


def set_map(G, xy, ty, cov=None):
    G.map_clear()
    if len(ty):
        G.map_append(xy, ty)
        if cov is not None:
            G.map_set_cov(0, cov)
    assert G.map_size() == len(ty)


def five_paths(pkg, G, c, prm, map_xy=None, map_ty=None, map_cov="case"):
    """{path: (idx, d2, second)} of the batch call (assoc_grid 0, 1, -1) and the resident call (grid, brute force); leaves the map resident"""
    map_xy = c["map_xy"] if map_xy is None else map_xy; map_ty = c["map_ty"] if map_ty is None else map_ty
    map_cov = c["map_cov"] if isinstance(map_cov, str) else map_cov
    out = {}
    for mode in (0, 1, -1):
        G.set_debug(assoc_grid=mode)
        out["batch grid=%d" % mode] = G.associate_nn(c["poses"], c["pose_of"], c["obs"], map_xy, map_ty, map_cov, c["pose_cov"], prm)
    set_map(G, map_xy, map_ty, map_cov)
    d = Dev(pkg, c["poses"], c["pose_of"], c["obs"], c["pose_cov"])
    out["resident grid"] = d.resident(G, prm)
    G.set_debug(assoc_grid=0)
    out["resident brute"] = d.resident(G, prm)
    G.set_debug(assoc_grid=-1)
    d.free()
    return out


def frame_path(G, c, prm):
    """gs_frame_frontend_nn pose by pose against the resident map, put back in the case's order"""
    n = len(c["obs"]); z = np.zeros((n, 2)); g = np.zeros((n, 2)); idx = np.zeros(n, dtype=np.int32); d2 = np.zeros(n); sec = np.zeros(n)
    for p in range(len(c["poses"])):
        sel = np.flatnonzero(np.asarray(c["pose_of"]) == p)
        if len(sel):
            z[sel], g[sel], idx[sel], d2[sel], sec[sel] = G.frame_frontend_nn(c["poses"][p], c["obs"][sel], None if c["pose_cov"] is None else c["pose_cov"][p], prm)
    return z, g, idx, d2, sec


def same_bits(a, b):
    return all(np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x, y.view(np.int64) if y.dtype == np.float64 else y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ns.NAMES)
def test_every_path_against_the_exact_reference(pkg, G, name):
    c = ns.case(name); R = ns.reference(name); prm = pkg.binding.nn_params(**c["params"])
    res = five_paths(pkg, G, c, prm)
    worst = {}
    for path, r in res.items():
        worst[path] = R.check(*r, tag=(name, path))
    first = res["batch grid=0"]
    assert all(same_bits(first, r) for r in res.values()), (name, "the batch and resident paths disagree", {k: [int((np.asarray(a) != np.asarray(b)).sum()) for a, b in zip(first, v)] for k, v in res.items()})
    z, g, idx, d2, sec = frame_path(G, c, prm)
    worst["frame"] = R.check(idx, d2, sec, tag=(name, "frame"))
    assert same_bits(first, (idx, d2, sec)), (name, "the frame path's bits differ", int((idx != first[0]).sum()), int((d2 != first[1]).sum()), int((sec != first[2]).sum()))
    A = R.R
    sz = fx.check_xy(z, A.z_hi, A.z_lo, A.Bz, A.nan, A.band, (name, "frame z")); sg = fx.check_xy(g, A.g_hi, A.g_lo, A.Bg, A.nan, A.band, (name, "frame g"))
    u = R.unique_answer()
    assert ((u == -2) | (u == first[0])).all()
    for i, j in c["notes"].get("expect", {}).items():
        assert first[0][i] == j, (name, i, int(first[0][i]), j)
    for i in c["notes"].get("alone", ()):
        assert first[0][i] >= 0 and np.isinf(first[2][i]), (name, i, "a lone cone has no runner-up", float(first[2][i]))
    if "without_pose_cov" in c["notes"]:
        c2 = dict(c); c2["pose_cov"] = None
        r2 = five_paths(pkg, G, c2, prm)
        for i, j in c["notes"]["without_pose_cov"].items():
            assert all(r[0][i] == j for r in r2.values()), (name, i, j)
    STATS[name] = (c["family"], worst, sz["worst"], sg["worst"])
    print("%-16s %-7s d2 / second worst: grid %.3f / %.3f  brute %.3f / %.3f  frame %.3f / %.3f | frame z %.3f g %.3f | matched %d of %d" %
          ((name, c["family"]) + worst["batch grid=1"] + worst["batch grid=0"] + worst["frame"] + (sz["worst"], sg["worst"], int((first[0] >= 0).sum()), len(idx))))
    G.map_clear()


def test_family_record():
    """the worst ratios per family of the cases that ran in this session (printed for the docstring's record; every one below 1 by the checker)"""
    fam = {}
    for name, (f, w, sz, sg) in STATS.items():
        cur = fam.setdefault(f, [0.0] * 8)
        vals = list(w["batch grid=0"]) + list(w["batch grid=1"]) + list(w["frame"]) + [sz, sg]
        fam[f] = [max(a, b) for a, b in zip(cur, vals)]
    for f, v in fam.items():
        print("%-8s k_assoc_nn %.3f / %.3f   k_assoc_nn_grid %.3f / %.3f   k_frame_nn %.3f / %.3f   frame z %.3f g %.3f" % ((f,) + tuple(v)))
        assert max(v) < 1.0


def test_gate_distance_and_tie_bit_for_bit_on_every_path(pkg, G):
    """S = I by construction (sigma_xy = 1, every other noise 0): d2 = fl(a'^2) exactly.  gate_chi2 = d2 gives -1, the next fp64 the cone; the
    same for max_distance = a'; two cones at g +- (a', 0) with equal covariance tie exactly: the lower index wins and second_d2 == d2"""
    base = dict(lidar=ns.LIDAR, poses=ns.EQ_POSE, pose_of=np.zeros(len(ns.EQ_OBS), dtype=np.int32), obs=ns.EQ_OBS, pose_cov=None)
    G.map_clear()
    _, g, _, _, _ = G.frame_frontend_nn(ns.EQ_POSE[0], ns.EQ_OBS)
    assert np.isfinite(g).all()
    n = 0
    for kind, i, xy, ty, cov, kw, ej, ed, es in ns.exact_cases(g):
        prm = pkg.binding.nn_params(**kw)
        res = five_paths(pkg, G, base, prm, xy, ty, cov)
        _, gf, idx, d2, sec = G.frame_frontend_nn(ns.EQ_POSE[0], ns.EQ_OBS, None, prm)
        assert np.array_equal(gf, g)
        res["frame"] = (idx, d2, sec)
        for path, r in res.items():
            assert r[0][i] == ej and r[1][i] == ed and r[2][i] == es, (kind, path, i, int(r[0][i]), ej, float(r[1][i]), ed, float(r[2][i]), es)
        n += 1
    assert n == 40
    G.map_clear()


def _resident_one(pkg, G, c, prm):
    d = Dev(pkg, c["poses"], c["pose_of"], c["obs"], c["pose_cov"]); r = d.resident(G, prm); d.free()
    return r


def test_resident_covariances_through_the_map_changes(pkg):
    """append (zeros) / set_cov / clear and re-append (zeros again) / growth across the 1024-cone capacity (kept) / a partial set / a refused set
    (nothing changes): gs_map_get_cov and one resident call after each step, the call against the batch result on the map as it should then be"""
    c = dict(ns.case("map1025")); prm = pkg.binding.nn_params(); xy, ty, cov = c["map_xy"], c["map_ty"], c["map_cov"]
    G = pkg.Graph(lidar_to_cog=ns.LIDAR)                                    # a handle of its own: its map starts without capacity and without covariances
    def check(m, expect_cov, what):
        got = G.map_cov(0, m).reshape(-1, 4)
        assert np.array_equal(got, expect_cov[:m]), what
        want = G.associate_nn(c["poses"], c["pose_of"], c["obs"], xy[:m], ty[:m], expect_cov[:m], c["pose_cov"], prm)
        assert same_bits(want, _resident_one(pkg, G, c, prm)), what
    zero = np.zeros_like(cov)
    G.map_clear(); G.map_append(xy[:600], ty[:600]); check(600, zero, "appended cones have zero covariance")
    G.map_set_cov(0, cov[:600]); check(600, cov, "set_cov")
    G.map_clear(); G.map_append(xy[:600], ty[:600]); check(600, zero, "clear drops the covariances")
    G.map_set_cov(0, cov[:600])
    G.map_append(xy[600:], ty[600:])                                       # 1025 cones: beyond the first capacity of 1024
    exp = cov.copy(); exp[600:] = 0.0; check(1025, exp, "growth keeps the covariances, the new cones have none")
    G.map_set_cov(1000, cov[1000:1025]); exp[1000:] = cov[1000:]; check(1025, exp, "a partial set_cov")
    G.map_set_xy(10, xy[10:20]); check(1025, exp, "set_xy leaves the covariances")
    bad = cov[:3].copy(); bad[2, 1] = np.nextafter(bad[2, 2], 1.0)          # the last block is not bitwise symmetric: nothing of the call is taken
    for blk in (bad, [[1.0, 0, 0, -1e-300]], [[np.nan, 0, 0, 1]], [[1, np.inf, np.inf, 1]]):
        with pytest.raises(pkg.binding.GsError) as e:
            G.map_set_cov(5, blk)
        assert e.value.code == -1
    with pytest.raises(pkg.binding.GsError) as e:
        G.map_set_cov(1024, cov[:2])                                       # beyond the end of the map
    assert e.value.code == -1
    check(1025, exp, "a refused set_cov changes nothing")
    G.close()


def test_map_covariances_from_the_marginals(pkg):
    from conftest import random_graph
    g = random_graph(7)                                                    # 40 poses / 25 landmarks, landmark 3 fixed (a zero block)
    H = pkg.Graph(); H.load_bench_graph(g); H.optimize(10); H.compute_marginals()
    S = H.landmark_covariances().reshape(-1, 4); M = len(S)
    H.map_append(H.landmarks(), np.ones(M, dtype=np.int32)); H.map_append(np.zeros((3, 2)), np.ones(3, dtype=np.int32))
    H.map_set_cov(0, np.tile([1.0, 0.0, 0.0, 1.0], (M + 3, 1)))
    ids = np.arange(M, dtype=np.int32)[::-1].copy(); ids[4] = -1
    H.map_set_cov_from_marginals(2, ids)
    got = H.map_cov().reshape(-1, 4); exp = np.tile([1.0, 0.0, 0.0, 1.0], (M + 3, 1)); exp[2:2 + M] = S[::-1]; exp[6] = 0.0
    assert np.array_equal(got.view(np.int64), exp.view(np.int64))          # bit-identical to gs_get_landmark_covariances; -1 gives zeros; the rest untouched
    with pytest.raises(pkg.binding.GsError) as e:
        H.map_set_cov_from_marginals(0, [10 ** 6])
    assert e.value.code == -3
    with pytest.raises(pkg.binding.GsError) as e:
        H.map_set_cov_from_marginals(M, np.arange(4))                     # beyond the end of the map
    assert e.value.code == -1
    H.iterate(); H.synchronize()
    with pytest.raises(pkg.binding.GsError) as e:
        H.map_set_cov_from_marginals(0, [0])
    assert e.value.code == -6                                              # stale marginals, as the getters
    assert np.array_equal(H.map_cov().reshape(-1, 4), exp)
    H.close()


def test_misaligned_observations_and_a_pose_index_out_of_range(pkg, G):
    c = dict(ns.case("map257")); prm = pkg.binding.nn_params()
    set_map(G, c["map_xy"], c["map_ty"], c["map_cov"])
    d = Dev(pkg, c["poses"], c["pose_of"], c["obs"], c["pose_cov"]); good = d.resident(G, prm)
    class Shifted:
        ptr = C.c_void_p(d.ob.ptr.value + 8)
    rc = pkg.binding.lib().gs_associate_nn_resident(G.h, d.n - 1, d.p.ptr, d.np, d.po.ptr, Shifted.ptr, None, C.byref(prm), d.idx.ptr, None, None)
    assert rc == -1
    d.free()
    po = np.array(c["pose_of"]); po[3] = len(c["poses"]); po[100] = -1; po[200] = 2 ** 31 - 1
    for grid in (-1, 0):
        G.set_debug(assoc_grid=grid)
        d = Dev(pkg, c["poses"], po, c["obs"], c["pose_cov"]); r = d.resident(G, prm); d.free()
        for i in (3, 100, 200):
            assert r[0][i] == -1 and np.isinf(r[1][i]) and np.isinf(r[2][i])
        keep = np.ones(len(po), dtype=bool); keep[[3, 100, 200]] = False
        assert same_bits([a[keep] for a in good], [a[keep] for a in r]), "the other observations changed"
    G.set_debug(assoc_grid=-1); G.map_clear()


def test_the_batch_call_skips_a_negative_definite_block(pkg, G):
    """det > 0 and S00 < 0 (all sigmas 0, the cone's block -I): gs_map_set_cov refuses such a block, the batch call takes what it is given and
    the S00 test skips the cone; the proper cone behind it is taken"""
    c = dict(ns.case("indefinite")); prm = pkg.binding.nn_params(**c["params"])
    cov = np.array(c["map_cov"]); cov[6] = (-1.0, 0.0, 0.0, -1.0); cov[3] = (-1.0, 0.0, 0.0, -1.0); cov[20] = (0.1, 0.0, 0.0, 0.1)
    xy = np.array(c["map_xy"]); ty = np.array(c["map_ty"]); xy[20] = xy[6] + (0.1, 0.0); ty[20] = ty[6]
    for mode in (0, 1, -1):
        G.set_debug(assoc_grid=mode)
        idx, d2, sec = G.associate_nn(c["poses"], c["pose_of"], c["obs"], xy, ty, cov, None, prm)
        assert idx[0] == 20 and np.isinf(sec[0]) and idx[1] == -1, (mode, idx[:2].tolist(), float(sec[0]))
    G.set_debug(assoc_grid=-1)


def test_the_euclidean_association_is_unchanged_by_nn_calls(pkg, G):
    """the resident grid is keyed on the radius: Euclidean calls (1.2 m) around NN calls (3 m, then 0.7 m) return the same indices as before"""
    c = dict(ns.case("map2047")); prm = pkg.binding.nn_params()
    set_map(G, c["map_xy"], c["map_ty"], c["map_cov"])
    DA = pkg.binding.DeviceArray; out = DA(nbytes=4 * len(c["obs"]))
    d = Dev(pkg, c["poses"], c["pose_of"], c["obs"], c["pose_cov"])
    def euclid():
        G.associate_resident(d.p, d.np, d.po, d.ob, d.n, 1.2, out); G.synchronize()
        return out.to_host(np.int32, d.n)
    before = euclid(); want = G.associate(c["poses"], c["pose_of"], c["obs"], c["map_xy"], c["map_ty"], 1.2)
    assert np.array_equal(before, want) and (before >= 0).any()
    a = d.resident(G, prm); assert np.array_equal(euclid(), before)
    b = d.resident(G, pkg.binding.nn_params(max_distance=0.7)); assert np.array_equal(euclid(), before)
    assert same_bits(a, d.resident(G, prm)) and (b[0] >= 0).sum() < (a[0] >= 0).sum()
    R = nr.make(dict(c, params=dict(max_distance=0.7))); R.check(*b, tag="max_distance 0.7")
    d.free(); out.free(); G.map_clear()
