"""GPU tests of the minimum-cost association (k_assign_opt / k_assign_opt_big of gs_assoc_nn.hip): a frame's cones matched at least total d2
over every observation's 8 best admissible cones.

The cases are the 25 of tests/assoc_nn_shapes.py with their observations grouped into frames by pose (test_assign_opt_cpu.py holds the census:
55 frames, all DECIDED by the exact reference, the greedy matching beaten in 14).  Every case runs through SIX paths — gs_assign_opt_batch with
assoc_grid 0, 1, -1, gs_assign_opt_resident with the grid and with brute force, gs_frame_frontend_assign_opt frame by frame — which must agree
bit for bit in index, d2 and n_admissible, and each is held to the exact reference (assign_opt_ref.FrameRef).  Independently of that reference
the optimum is evaluated exactly on THE DEVICE'S OWN d2(i, j), rebuilt from single-cone gs_associate_nn_batch calls as test_gpu_assign_nn.py
does: where the margin to the best different matching exceeds T the indices and d2 bits must be equal, everywhere the total gain must be within
T of the optimum.  T(k) = 48 k^2 2^-53 gate_chi2 is derived in assign_opt_ref.py from the solver's operation count, not measured.  The result
is cross-checked against gs_associate_nn_batch (frames without a duplicate there) and gs_assign_nn_batch (frames where the greedy is optimal,
and the total gain everywhere).  Scenes with S = I are exact by construction: every d2 is reproducible in numpy from the path's own global XY.

Measured on an MI355X: all 55 frames decided and equal to the exact optimum on all six paths; on the device's own distances every frame's
margin exceeds T and the indices are equal (528 single-cone calls for map2047, the most), (optimum - gain) / T is 0 in every frame and in
every exact scene, the tie scenes included; the file runs in under five seconds."""
import ctypes as C

import numpy as np
import pytest

import assign_nn_ref as ar
import assign_opt_ref as ao
import assoc_exec as ax
import assoc_nn_shapes as ns

pytestmark = pytest.mark.gpu
PATHS = ("batch grid=0", "batch grid=1", "batch grid=-1", "resident grid", "resident brute", "frame")
FILL_I, FILL_D, FILL_N = 12345, 777.0, 54321


@pytest.fixture(scope="module")
def G(pkg):
    if pkg.device_count() < 1:
        pytest.fail("no gfx950 device visible: the HIP path cannot run")
    g = pkg.Graph(lidar_to_cog=ns.LIDAR)
    yield g
    g.close()


def bits(a):
    a = np.asarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same_bits(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def set_map(G, xy, ty, cov=None):
    G.map_clear()
    if len(ty):
        G.map_append(xy, ty)
        if cov is not None:
            G.map_set_cov(0, cov)
    assert G.map_size() == len(ty)


class Dev:
    """poses, pose indices, observations, frame offsets and pose covariances in device memory; the three outputs pre-filled with a pattern"""

    def __init__(self, pkg, poses, pose_of, obs, frame_start, pose_cov=None, n_poses=None):
        DA = pkg.binding.DeviceArray; f = lambda a, t: DA(np.ascontiguousarray(a, dtype=t))
        self.n = len(obs); self.np = len(poses) if n_poses is None else n_poses; self.nf = len(frame_start) - 1
        self.p, self.po, self.ob, self.fs = f(poses, np.float64), f(pose_of, np.int32), f(obs, np.float64), f(frame_start, np.int32)
        self.pc = None if pose_cov is None else f(pose_cov, np.float64)
        self.idx, self.d2, self.na = f(np.full(self.n, FILL_I), np.int32), f(np.full(self.n, FILL_D), np.float64), f(np.full(self.n, FILL_N), np.int32)

    def assign(self, G, params):
        G.assign_opt_resident(self.p, self.np, self.po, self.ob, self.n, self.nf, self.fs, self.idx, self.d2, self.na, self.pc, params); G.synchronize()
        return self.idx.to_host(np.int32, self.n), self.d2.to_host(np.float64, self.n), self.na.to_host(np.int32, self.n)

    def greedy(self, G, params):
        G.assign_nn_resident(self.p, self.np, self.po, self.ob, self.n, self.nf, self.fs, self.idx, self.d2, self.pc, params); G.synchronize()
        return self.idx.to_host(np.int32, self.n), self.d2.to_host(np.float64, self.n)

    def free(self):
        for a in (self.p, self.po, self.ob, self.fs, self.pc, self.idx, self.d2, self.na):
            if a is not None:
                a.free()


def six_paths(pkg, G, poses, pose_of, obs, fs, xy, ty, cov, pose_cov, prm):
    """{path: (idx, d2, n_admissible)} in the order of `obs`; every frame of fs must hold one pose's observations (the frame call takes one pose)"""
    out = {}
    for mode in (0, 1, -1):
        G.set_debug(assoc_grid=mode)
        out["batch grid=%d" % mode] = G.assign_opt(poses, pose_of, obs, fs, xy, ty, cov, pose_cov, prm)
    set_map(G, xy, ty, cov)
    d = Dev(pkg, poses, pose_of, obs, fs, pose_cov)
    out["resident grid"] = d.assign(G, prm)
    G.set_debug(assoc_grid=0)
    out["resident brute"] = d.assign(G, prm)
    G.set_debug(assoc_grid=-1)
    d.free()
    n = len(obs); idx = np.full(n, FILL_I, dtype=np.int32); d2 = np.full(n, FILL_D); na = np.full(n, FILL_N, dtype=np.int32)
    for f in range(len(fs) - 1):
        a, b = int(fs[f]), int(fs[f + 1])
        if b > a:
            p = int(pose_of[a]); assert (np.asarray(pose_of[a:b]) == p).all()
            _, _, idx[a:b], d2[a:b], na[a:b] = G.frame_frontend_assign_opt(poses[p], obs[a:b], None if pose_cov is None else pose_cov[p], prm)
    out["frame"] = (idx, d2, na)
    assert tuple(out) == PATHS
    return out


def all_agree(res, tag):
    first = res[PATHS[0]]
    for path, r in res.items():
        assert same_bits(first, r), (tag, path, "differs from", PATHS[0], int((r[0] != first[0]).sum()), int((bits(r[1]) != bits(first[1])).sum()), int((r[2] != first[2]).sum()))
    return first


def gain(idx, d2, gate):
    """the exact total gain of a frame's result from its own d2"""
    return sum((ao.frac(gate) - ao.frac(float(d)) for j, d in zip(idx, d2) if j >= 0), ao.frac(0))


@pytest.fixture(scope="module")
def runs(pkg, G):
    """the six paths of a case, framed by pose, computed once and shared: name -> (order, frame_start, framed case arrays, results)"""
    memo = {}
    def get(name):
        if name not in memo:
            c = ns.case(name); order, fs = ar.frames_by_pose(c["pose_of"])
            po = np.ascontiguousarray(c["pose_of"][order]); ob = np.ascontiguousarray(c["obs"][order])
            prm = pkg.binding.nn_params(**c["params"])
            res = six_paths(pkg, G, c["poses"], po, ob, fs, c["map_xy"], c["map_ty"], c["map_cov"], c["pose_cov"], prm)
            G.map_clear()
            memo[name] = (order, fs, po, ob, prm, res)
        return memo[name]
    return get


_refs = {}


def frame_refs(name, order, fs):
    """the exact reference's frames of a case, computed once and shared (and never changed)"""
    if name not in _refs:
        R = ns.reference(name)
        _refs[name] = [ao.FrameRef(R, order[int(fs[f]):int(fs[f + 1])]) for f in range(len(fs) - 1)]
    return _refs[name]


@pytest.mark.parametrize("name", ns.NAMES)
def test_every_case_on_every_path_against_the_exact_reference(runs, name):
    order, fs, po, ob, prm, res = runs(name)
    first = all_agree(res, name)
    decided = differs = 0
    for f, F in enumerate(frame_refs(name, order, fs)):
        a, b = int(fs[f]), int(fs[f + 1])
        for path, r in res.items():
            bad = F.failures(r[0][a:b], r[1][a:b], r[2][a:b])
            assert not bad, (name, path, "frame %d" % f, bad[0], "%d fail" % len(bad))
        decided += F.decided; differs += F.greedy()[0] != F.expect
    print("%-16s frames %d decided %d optimum differs from the greedy in %d matched %d of %d" % (name, len(fs) - 1, decided, differs, int((first[0] >= 0).sum()), len(ob)))
    assert decided == len(fs) - 1                                          # (the census of test_assign_opt_cpu.py: every frame's indices are the exact optimum's)


def device_matrix(G, c, po, ob, prm, cones):
    """D[i, c] = the device's own bits of d2(i, cones[c]), +inf where the pair is not admissible: gs_associate_nn_batch against that cone alone"""
    D = np.full((len(ob), len(cones)), np.inf)
    for col, j in enumerate(cones):
        idx, d2, _ = G.associate_nn(c["poses"], po, ob, c["map_xy"][j:j + 1], c["map_ty"][j:j + 1], None if c["map_cov"] is None else c["map_cov"][j:j + 1], c["pose_cov"], prm)
        assert ((idx == 0) == np.isfinite(d2)).all()
        D[:, col] = d2
    return D


def hold_to_matrix(D, cones, res, gate, tag):
    """a frame's result against the exact optimum over the matrix D of fp64 distances; returns (optimum - gain) / T and whether the margin decided it"""
    idx, d2, na = res; k = len(D)
    rows = ao.cut(ao.rows_of(D, cones)); best, expect = ao.solve(rows, gate); mg = ao.margin(rows, gate); T = ao.T(k, gate)
    assert np.array_equal(na, np.isfinite(D).sum(axis=1)), (tag, "n_admissible")
    v = ao.value(rows, [int(j) for j in idx], gate)                         # (asserts a matching over pairs of the cut lists)
    col = {j: c for c, j in enumerate(cones)}
    want = [D[i, col[int(j)]] if j >= 0 else np.inf for i, j in enumerate(idx)]
    assert np.array_equal(bits(np.array(want, dtype=np.float64)), bits(d2)), (tag, "d2 is not the pair's")
    assert best - v <= T, (tag, "total gain below the optimum by", float(best - v), "T", float(T))
    if mg > T:
        assert [int(j) for j in idx] == expect, (tag, "index", [int(j) for j in idx][:12], expect[:12])
    return (float((best - v) / T) if k else 0.0), mg > T


@pytest.mark.parametrize("name", ns.NAMES)
def test_the_optimum_over_the_devices_own_distances(G, runs, name):
    order, fs, po, ob, prm, res = runs(name); R = ns.reference(name); c = ns.case(name)
    first = res[PATHS[0]]
    frames = range(len(fs) - 1) if name != "random2048" else range(2)     # (a few hundred single-cone calls at the most)
    calls = by_margin = 0; worst = 0.0
    for f in frames:
        a, b = int(fs[f]), int(fs[f + 1])
        cones = sorted({cd.j for i in order[a:b] for cd in R.cands[int(i)]})
        D = device_matrix(G, c, po[a:b], ob[a:b], prm, cones); calls += len(cones)
        w, m = hold_to_matrix(D, cones, tuple(x[a:b] for x in first), prm.gate_chi2, (name, f)); worst = max(worst, w); by_margin += m
    print("%-16s %d single-cone calls, %d of %d frames held to equal indices, worst (optimum - gain) / T %.3g" % (name, calls, by_margin, len(frames), worst))
    assert calls <= 600                                                    # (a guard on the test's own cost: map2047 needs 528)


@pytest.mark.parametrize("name", ns.NAMES)
def test_cross_checks_against_the_existing_calls(G, runs, name):
    order, fs, po, ob, prm, res = runs(name); c = ns.case(name)
    first = res[PATHS[0]]
    nn = G.associate_nn(c["poses"], po, ob, c["map_xy"], c["map_ty"], c["map_cov"], c["pose_cov"], prm)
    gr = G.assign_nn(c["poses"], po, ob, fs, c["map_xy"], c["map_ty"], c["map_cov"], c["pose_cov"], prm)
    same = as_greedy = better = 0
    for f, F in enumerate(frame_refs(name, order, fs)):
        a, b = int(fs[f]), int(fs[f + 1])
        if not ar.has_duplicates(nn[0][a:b]):
            same += 1
            assert same_bits((nn[0][a:b], nn[1][a:b]), (first[0][a:b], first[1][a:b])), (name, f, "differs from gs_associate_nn_batch")
        if F.greedy()[0] == F.expect:
            as_greedy += 1
            assert same_bits((gr[0][a:b], gr[1][a:b]), (first[0][a:b], first[1][a:b])), (name, f, "differs from gs_assign_nn_batch")
        if (first[2][a:b] <= ao.CAND_MAX).all():
            go, gg = gain(first[0][a:b], first[1][a:b], prm.gate_chi2), gain(gr[0][a:b], gr[1][a:b], prm.gate_chi2)
            assert go >= gg, (name, f, float(go), float(gg))
            better += go > gg
    print("%-16s frames equal to gs_associate_nn_batch %d, equal to gs_assign_nn_batch %d, with a larger gain than it %d" % (name, same, as_greedy, better))


# ---- exact by construction: S = I (sigma_xy = 1, the other sigmas 0, no covariances), so d2 = fl(fl(nu0^2) + fl(nu1^2)) in numpy as on the device
def exact_matrix(g, oty, xy, ty, prm):
    """the header's pair formula for S = I, operation by operation, from the device's own global XY"""
    g = np.asarray(g); xy = np.asarray(xy, dtype=np.float64)
    n0 = xy[None, :, 0] - g[:, None, 0]; n1 = xy[None, :, 1] - g[:, None, 1]
    s = n0 * n0 + n1 * n1
    ok = (np.abs(np.asarray(ty, dtype=np.float64)[None, :] - np.asarray(oty)[:, None]) < prm.type_tol) & (np.sqrt(s) < prm.max_distance) & (s < prm.gate_chi2)
    return np.where(ok, s, np.inf)


WORST = {}


def run_exact(pkg, G, obs, xy, ty, tag, **kw):
    """the six paths of one frame of `obs` seen from EQ_POSE against (xy, ty), held to the exact optimum over the numpy matrix D; (D, idx, d2, na)"""
    obs = np.ascontiguousarray(obs, dtype=np.float64); k = len(obs); xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2); ty = np.asarray(ty, dtype=np.int32)
    prm = pkg.binding.nn_params(**dict(ns.EQ_SIGMAS, **kw))
    set_map(G, xy, ty)
    zn, g, _, _, _ = G.frame_frontend_nn(ns.EQ_POSE[0], obs, None, prm)
    z, g2, _, _, _ = G.frame_frontend_assign_opt(ns.EQ_POSE[0], obs, None, prm)
    assert same_bits((zn, g), (z, g2)), (tag, "z / g are not gs_frame_frontend_nn's bits")
    D = exact_matrix(g, obs[:, 3], xy, ty, prm)
    res = six_paths(pkg, G, ns.EQ_POSE, np.zeros(k, dtype=np.int32), obs, np.array([0, k], dtype=np.int32), xy, ty, None, None, prm)
    first = all_agree(res, tag)
    WORST[tag], _ = hold_to_matrix(D, list(range(len(ty))), first, prm.gate_chi2, tag)
    G.map_clear()
    return D, [int(j) for j in first[0]], first[1], first[2]


def device_g(G, obs):
    G.map_clear()
    return G.frame_frontend_nn(ns.EQ_POSE[0], np.ascontiguousarray(obs, dtype=np.float64))[1]


def obs_at(G, targets, ty):
    """observations [k, 4] (zenith 0) whose global XY from EQ_POSE is `targets` to within a micrometre: Newton on the numpy A0, checked on the device"""
    t = ns.EQ_POSE[0]; c, s = np.cos(t[2]), np.sin(t[2]); out = []
    for gt in np.asarray(targets, dtype=np.float64):
        d = gt - t[:2]; zt = np.array([c * d[0] + s * d[1], -s * d[0] + c * d[1]])
        x = np.array([np.degrees(np.arctan2(zt[1], zt[0])), np.hypot(*zt)])
        f = lambda x: ax.polar_to_xy(x[0], 0.0, x[1], ns.LIDAR) - zt
        for _ in range(30):
            r = f(x); J = np.stack([(f(x + h) - r) / 1e-6 for h in (np.array([1e-6, 0.0]), np.array([0.0, 1e-6]))], axis=1)
            x = x - np.linalg.solve(J, r)
        out.append([x[0], 0.0, x[1], ty])
    out = np.array(out); g = device_g(G, out)
    assert np.abs(g - np.asarray(targets)).max() < 1e-6 and (np.abs(out[:, 0]) > 1.0).all() and (np.abs(out[:, 0]) < 85.0).all(), out
    return out


def test_exact_the_two_by_two(pkg, G):
    """d2 = [[a, c], [b, -]] with a < b < c and gate > b + c - a: the greedy takes (0, 0) and leaves observation 1 without a cone, the optimum is
    (0, 1), (1, 0).  The '-' comes from the types (2 and 1 against cones of type 2 and 3 with type_tol 1.5)"""
    base = ns.EQ_OBS[0]; obs = np.array([base, base]); obs[1, 2] += 0.05; obs[:, 3] = (2, 1)
    g = device_g(G, obs); u = (g[1] - g[0]) / np.hypot(*(g[1] - g[0]))
    xy = [g[0] - 1.0 * u, g[0] + 1.4 * np.array([-u[1], u[0]])]
    D, idx, d2, na = run_exact(pkg, G, obs, xy, [2, 3], "2 x 2", type_tol=1.5, gate_chi2=5.99)
    assert np.isinf(D[1, 1]) and D[0, 0] < D[1, 0] < D[0, 1] and D[1, 0] + D[0, 1] - D[0, 0] < 5.99, D
    assert ar.greedy(D)[0] == [0, -1] and idx == [1, 0] and na.tolist() == [2, 1]


def test_exact_three_observations_on_two_cones(pkg, G):
    base = ns.EQ_OBS[1]; obs = np.tile(base, (3, 1)); obs[:, 2] += (0.0, 0.4, 0.8)
    g = device_g(G, obs); u = (g[2] - g[0]) / np.hypot(*(g[2] - g[0]))
    xy = [g[1] - 0.15 * u, g[1] + 0.17 * u]                                # both cones between observations 0 and 2; observation 1 is nearest to both
    D, idx, d2, na = run_exact(pkg, G, obs, xy, [3, 3], "3 on 2", gate_chi2=5.99)
    assert np.isfinite(D).all() and D[1, 0] < D[0, 0] and D[1, 1] < D[2, 1], D
    assert sorted(j for j in idx if j >= 0) == [0, 1] and idx.count(-1) == 1 and na.tolist() == [2, 2, 2]


def test_exact_a_chain_of_five(pkg, G):
    """observation i sees cone i + 1 at 0.45 and cone i at 0.55 (max_distance 0.8 hides the rest), observation 4 only cone 4: observations
    0 .. 3 take cones 1 .. 4, and adding observation 4 shifts every one of them down by one cone — an augmenting path through all five"""
    base = ns.EQ_OBS[1]; obs = np.tile(base, (5, 1)); obs[:, 2] += 1.0 * np.arange(5)
    g = device_g(G, obs); u = (g[4] - g[0]) / np.hypot(*(g[4] - g[0]))
    xy = [g[j] - 0.55 * u for j in range(5)]
    D, idx, d2, na = run_exact(pkg, G, obs, xy, [3] * 5, "chain", gate_chi2=5.99, max_distance=0.8)
    assert all(np.isfinite(D[i, i]) and (i == 4 or D[i, i + 1] < D[i, i]) for i in range(5)) and np.isfinite(D).sum() == 9, D
    assert ar.greedy(D)[0] == [1, 2, 3, 4, -1] and idx == [0, 1, 2, 3, 4] and na.tolist() == [2, 2, 2, 2, 1]


def test_exact_ties_with_two_optima(pkg, G):
    """two identical observations and two cones: (0, 0), (1, 1) and (0, 1), (1, 0) have the same total — either is right, by value"""
    base = ns.EQ_OBS[2]; two = np.array([base, base]); g = device_g(G, two)
    assert np.array_equal(bits(g[0]), bits(g[1]))
    D, idx, d2, na = run_exact(pkg, G, two, [g[0] + (0.6, 0.1), g[0] + (0.3, 0.1)], [1, 1], "two optima", gate_chi2=100.0)
    assert D[0, 0] == D[1, 0] and D[0, 1] == D[1, 1] and sorted(idx) == [0, 1]
    D, idx, d2, na = run_exact(pkg, G, two, [g[0] + (0.3, 0.1)], [1], "two observations, one cone", gate_chi2=100.0)
    assert sorted(idx) == [-1, 0] and na.tolist() == [1, 1]


def _tie_offsets(gx):
    for a in (1.0, 0.5, 2.0, 0.25):
        m1, a1 = ns._offset(gx, a); m2 = gx - a1
        if m2 - gx == -a1:
            return m1, m2, a1
    raise AssertionError("no power of two gives an exact pair of offsets")


def test_exact_a_pair_at_the_gate(pkg, G):
    """two identical observations, a near cone and one at d2 = a'^2 exactly.  gate == d2: the far pair is out and one observation stays without a
    cone.  gate = the next fp64: it is in, and it is matched although its gain is one ulp of the gate"""
    base = ns.EQ_OBS[3]; two = np.array([base, base]); g = device_g(G, two); m1, _, a1 = _tie_offsets(g[0, 0]); d = a1 * a1
    xy = [(g[0, 0] + 0.125, g[0, 1]), (m1, g[0, 1])]
    D, idx, d2, na = run_exact(pkg, G, two, xy, [4, 4], "gate, equal", gate_chi2=d)
    assert sorted(idx) == [-1, 0] and np.isinf(D[:, 1]).all() and na.tolist() == [1, 1]
    D, idx, d2, na = run_exact(pkg, G, two, xy, [4, 4], "gate, next", gate_chi2=float(np.nextafter(d, np.inf)))
    assert sorted(idx) == [0, 1] and (D[:, 1] == d).all() and sorted(d2.tolist()) == sorted([D[0, 0], d]) and na.tolist() == [2, 2]


def test_exact_the_cut_to_eight_candidates(pkg, G):
    """observation 0 has 9 admissible cones; the nearest 8 are each the only candidate of another observation, the 9th is free but not on its
    list: it gets -1 and n_admissible = 9"""
    g0 = device_g(G, ns.EQ_OBS[:1])[0]; ang = np.radians(40.0 * np.arange(9) + 100.0); dirs = np.stack([np.cos(ang), np.sin(ang)], axis=1)
    obs = np.concatenate([ns.EQ_OBS[:1], obs_at(G, g0 + 4.0 * dirs[:8], ns.EQ_OBS[0, 3])])
    xy = np.concatenate([g0 + (2.1 + 0.01 * np.arange(8))[:, None] * dirs[:8], [g0 + 2.3 * dirs[8]]])      # (each nearer to its own observation, 4 m out, than to observation 0)
    D, idx, d2, na = run_exact(pkg, G, obs, xy, [int(ns.EQ_OBS[0, 3])] * 9, "cut", gate_chi2=100.0, max_distance=2.5)
    assert np.isfinite(D[0]).all() and (np.diff(D[0]) > 0).all() and all(np.isfinite(D[i]).tolist() == [j == i - 1 for j in range(9)] for i in range(1, 9)), D
    assert idx == [-1] + list(range(8)) and na.tolist() == [9] + [1] * 8
    assert ao.solve(ao.rows_of(D), 100.0)[1] == [8] + list(range(8))       # (without the cut it would take the 9th)


def test_exact_256_identical_observations_against_256_cones(pkg, G):
    """every observation has the same 8 candidates: exactly 8 are matched, to those 8 cones, and every count is 256"""
    obs = np.tile(ns.EQ_OBS[0], (256, 1)); g = device_g(G, obs[:1])
    rng = np.random.default_rng(9); r = 0.05 + 0.01 * rng.permutation(256); th = rng.uniform(0, 2 * np.pi, 256)
    xy = g[0] + np.stack([r * np.cos(th), r * np.sin(th)], axis=1)
    D, idx, d2, na = run_exact(pkg, G, obs, xy, [2] * 256, "256 x 256", gate_chi2=100.0)
    assert len(np.unique(D[0])) == 256 and np.isfinite(D).all()
    assert sorted(j for j in idx if j >= 0) == sorted(np.argsort(D[0])[:8].tolist()) and idx.count(-1) == 248 and (na == 256).all()
    print("worst (optimum - gain) / T over the exact scenes: %s" % {k: "%.3g" % v for k, v in WORST.items()})


# ---- frames, defences, the other calls
def crowded(seed, n, n_cones):
    """one pose, n observations of one type and n_cones cones each 0.5 m (sigma) from some observation: more observations than cones, contests everywhere"""
    rng = np.random.default_rng(seed); poses = np.array([[2.0, -1.0, 0.4]]); ob = ns._obs(rng, n); ob[:, 3] = 1.0
    g = ax.cone_to_global(poses, np.zeros(n, dtype=np.int32), ob, ns.LIDAR)
    xy = g[rng.permutation(n)[:n_cones]] + rng.normal(size=(n_cones, 2)) * 0.5
    return poses, ob, xy, np.ones(n_cones, dtype=np.int32), ns.spd(rng, n_cones)


def test_frames_do_not_interact(pkg, G):
    sizes = (0, 1, 63, 64, 65, 255, 256); fs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    poses, base, xy, ty, cov = crowded(11, 256, 128)
    ob = np.concatenate([base[:s] for s in sizes]); po = np.zeros(len(ob), dtype=np.int32); prm = pkg.binding.nn_params()
    res = six_paths(pkg, G, poses, po, ob, fs, xy, ty, cov, None, prm)
    first = all_agree(res, "frames")
    gr = G.assign_nn(poses, po, ob, fs, xy, ty, cov, None, prm)
    for f, s in enumerate(sizes):
        a, b = int(fs[f]), int(fs[f + 1])
        alone = G.assign_opt(poses, po[a:b], ob[a:b], [0, s], xy, ty, cov, None, prm)
        assert same_bits(alone, tuple(x[a:b] for x in first)), ("frame of %d" % s)
        assert not ar.has_duplicates(first[0][a:b])
        if (first[2][a:b] <= ao.CAND_MAX).all():
            assert gain(first[0][a:b], first[1][a:b], prm.gate_chi2) >= gain(gr[0][a:b], gr[1][a:b], prm.gate_chi2), s
    a, b = int(fs[-2]), int(fs[-1])
    assert (first[0][a:b] != gr[0][a:b]).any(), "the frame of 256 is not one where the optimum differs from the greedy"
    G.map_clear()


def test_small_frames_share_a_wave_with_large_ones(pkg, G):
    """139 frames of mean size 4.5: a wave takes eight consecutive frames, side by side in 8 lanes each where they fit, in 16 / 32 / 64 lanes and
    several passes where one of the eight is larger (16, 33); the frame of 256 goes to the second kernel.  Every frame returns what it returns alone"""
    sizes = [1] * 60 + [256] + [2] * 40 + [16, 3, 8, 9, 7, 33, 0, 4] + [5] * 30; fs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    assert len(sizes) == 139 and fs[-1] <= 8 * len(sizes)
    poses, base, xy, ty, cov = crowded(13, 256, 128); rng = np.random.default_rng(13)
    starts = [int(rng.integers(0, 257 - s)) for s in sizes]                # every frame a window of the same 256 observations: they share cones
    ob = np.concatenate([base[st:st + s] for st, s in zip(starts, sizes)]); po = np.zeros(len(ob), dtype=np.int32); prm = pkg.binding.nn_params()
    res = six_paths(pkg, G, poses, po, ob, fs, xy, ty, cov, None, prm)
    first = all_agree(res, "mixed frames")
    gr = G.assign_nn(poses, po, ob, fs, xy, ty, cov, None, prm)
    moved = 0
    for f, s in enumerate(sizes):
        a, b = int(fs[f]), int(fs[f + 1])
        alone = G.assign_opt(poses, po[a:b], ob[a:b], [0, s], xy, ty, cov, None, prm)
        assert same_bits(alone, tuple(x[a:b] for x in first)), ("frame %d of %d" % (f, s))
        moved += not np.array_equal(gr[0][a:b], first[0][a:b])
    assert moved >= 1, "no frame where the optimum differs from the greedy"
    G.map_clear()


def test_an_empty_map(pkg, G):
    poses, base, xy, ty, cov = crowded(14, 40, 8); po = np.zeros(40, dtype=np.int32); prm = pkg.binding.nn_params()
    res = six_paths(pkg, G, poses, po, base, np.array([0, 7, 40], dtype=np.int32), np.zeros((0, 2)), np.zeros(0, dtype=np.int32), None, None, prm)
    first = all_agree(res, "empty map")
    assert (first[0] == -1).all() and np.isinf(first[1]).all() and (first[2] == 0).all()
    G.map_clear()


def test_invalid_queries_inside_a_contested_frame(pkg, G):
    """azimuth 0 (a NaN query) on every path; a pose index out of range on the resident path, which the host cannot see.  Either observation gets
    -1, +inf and 0 and takes part in nothing: the rest of the frame is what it is without it"""
    poses, base, xy, ty, cov = crowded(15, 48, 20); po = np.zeros(48, dtype=np.int32); prm = pkg.binding.nn_params(); fs = np.array([0, 48], dtype=np.int32)
    whole = G.assign_opt(poses, po, base, fs, xy, ty, cov, None, prm)
    v = int(np.flatnonzero(whole[0] >= 0)[3]); rest = np.arange(48) != v
    without = G.assign_opt(poses, po[rest], base[rest], [0, 47], xy, ty, cov, None, prm)
    assert ar.has_duplicates(G.associate_nn(poses, po[rest], base[rest], xy, ty, cov, None, prm)[0]), "the frame is not contested"
    ob = base.copy(); ob[v, 0] = 0.0
    first = all_agree(six_paths(pkg, G, poses, po, ob, fs, xy, ty, cov, None, prm), "azimuth 0")
    assert first[0][v] == -1 and np.isinf(first[1][v]) and first[2][v] == 0 and same_bits(tuple(x[rest] for x in first), without)
    set_map(G, xy, ty, cov)
    bad = po.copy(); bad[v] = 1
    for grid in (-1, 0):
        G.set_debug(assoc_grid=grid)
        for pv in (1, -1, 2 ** 30):
            bad[v] = pv
            d = Dev(pkg, poses, bad, base, fs); r = d.assign(G, prm); d.free()
            assert r[0][v] == -1 and np.isinf(r[1][v]) and r[2][v] == 0 and same_bits(tuple(x[rest] for x in r), without), (grid, pv)
    G.set_debug(assoc_grid=-1); G.map_clear()


def test_resident_defences(pkg, G):
    """a frame of 257 gets -1 / +inf / 0; frames with bounds outside [0, n] or a > b, and uncovered observations, leave the pre-filled pattern in all
    three outputs; the good frames between them return what they return alone"""
    n = 420; poses, base, xy, ty, cov = crowded(12, n, 200); po = np.zeros(n, dtype=np.int32); prm = pkg.binding.nn_params()
    bad = [0, 257, 300, 340, 700, 350, -5, 345]
    for grid, fs, good in ((-1, bad + [400], [(257, 300), (300, 340), (345, 400)]), (0, bad + [400], [(257, 300), (300, 340), (345, 400)]),
                           (-1, bad + list(range(346, 401)), [(257, 300), (300, 340)] + [(i, i + 1) for i in range(345, 400)])):   # (the last: 62 frames, eight to a wave)
        fs = np.array(fs, dtype=np.int32)
        G.set_debug(assoc_grid=grid)
        set_map(G, xy, ty, cov)
        d = Dev(pkg, poses, po, base, fs, None); idx, d2, na = d.assign(G, prm)
        assert (idx[:257] == -1).all() and np.isinf(d2[:257]).all() and (na[:257] == 0).all()
        written = np.zeros(n, dtype=bool); written[:257] = True
        for a, b in good:
            alone = G.assign_opt(poses, po[a:b], base[a:b], [0, b - a], xy, ty, cov, None, prm)
            assert same_bits(alone, (idx[a:b], d2[a:b], na[a:b])), (grid, a, b)
            assert b - a == 1 or (alone[0] >= 0).any()
            written[a:b] = True
        assert (idx[~written] == FILL_I).all() and (d2[~written] == FILL_D).all() and (na[~written] == FILL_N).all() and (~written).sum() == 25
        lib = pkg.binding.lib()                                              # the optional outputs left out: the index alone is written, and the same
        only = pkg.binding.DeviceArray(np.full(n, FILL_I, dtype=np.int32))
        assert lib.gs_assign_opt_resident(G.h, n, d.p.ptr, 1, d.po.ptr, d.ob.ptr, d.nf, d.fs.ptr, None, C.byref(prm), only.ptr, None, None) == 0
        G.synchronize(); assert np.array_equal(only.to_host(np.int32, n), idx); only.free()
        shifted = C.c_void_p(d.ob.ptr.value + 8)
        assert lib.gs_assign_opt_resident(G.h, n - 1, d.p.ptr, 1, d.po.ptr, shifted, d.nf, d.fs.ptr, None, C.byref(prm), d.idx.ptr, None, None) == -1
        d.free()
    G.set_debug(assoc_grid=-1); G.map_clear()


def test_the_existing_calls_are_unchanged_by_opt_calls(pkg, G):
    """every existing association call — Euclidean, nearest cone, greedy; resident, batch and frame — returns the same bits before and after
    minimum-cost calls on the handle (which re-key the resident grid on their own max_distance, as the others do)"""
    c = dict(ns.case("map2047")); prm = pkg.binding.nn_params(); order, fs = ar.frames_by_pose(c["pose_of"])
    po = np.ascontiguousarray(c["pose_of"][order]); ob = np.ascontiguousarray(c["obs"][order])
    set_map(G, c["map_xy"], c["map_ty"], c["map_cov"])
    DA = pkg.binding.DeviceArray; n = len(ob); k0 = int(fs[1])
    d = Dev(pkg, c["poses"], po, ob, fs, c["pose_cov"]); eo = DA(nbytes=4 * n); ni, nd, nsec = DA(nbytes=4 * n), DA(nbytes=8 * n), DA(nbytes=8 * n)
    def existing():
        G.associate_resident(d.p, d.np, d.po, d.ob, n, 1.2, eo)
        G.associate_nn_resident(d.p, d.np, d.po, d.ob, n, ni, nd, nsec, d.pc, prm); G.synchronize()
        out = (eo.to_host(np.int32, n), ni.to_host(np.int32, n), nd.to_host(np.float64, n), nsec.to_host(np.float64, n))
        out += tuple(G.frame_frontend_nn(c["poses"][0], ob[:k0], c["pose_cov"][0], prm)) + d.greedy(G, prm)
        out += tuple(G.frame_frontend_assign(c["poses"][0], ob[:k0], c["pose_cov"][0], prm))
        out += tuple(G.assign_nn(c["poses"], po, ob, fs, c["map_xy"], c["map_ty"], c["map_cov"], c["pose_cov"], prm))
        return out + tuple(G.associate_nn(c["poses"], po, ob, c["map_xy"], c["map_ty"], c["map_cov"], c["pose_cov"], prm))
    before = existing()
    assert (before[0] >= 0).any() and (before[1] >= 0).any()
    a = d.assign(G, prm); assert same_bits(existing(), before)
    b = d.assign(G, pkg.binding.nn_params(max_distance=0.7)); assert same_bits(existing(), before)
    G.frame_frontend_assign_opt(c["poses"][0], ob[:k0], c["pose_cov"][0], prm); assert same_bits(existing(), before)
    G.assign_opt(c["poses"], po, ob, fs, c["map_xy"], c["map_ty"], c["map_cov"], c["pose_cov"], prm); assert same_bits(existing(), before)
    assert same_bits(a, d.assign(G, prm)) and (b[0] >= 0).sum() < (a[0] >= 0).sum()
    for x in (d, eo, ni, nd, nsec):
        x.free()
    G.map_clear()
