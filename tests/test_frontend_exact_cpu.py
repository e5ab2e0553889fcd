"""CPU tests of the front-end test machinery: the cases of frontend_shapes.py reach what they are meant to reach, the reference of
frontend_exact_ref.py admits numpy and the CPU oracle everywhere, and the planted mistakes of assoc_exec.py are caught — so the same
checks, run on the device in test_gpu_frontend_exact.py, have teeth.

Recorded here (printed by the tests, -s):
  worst |got - exact| / B over every case: numpy 0.27 (z) and 0.49 (g), the CPU oracle the same (outside the branch band; inside it, as
  numbers, 0.34); of the 1280 branch-band entries numpy returns NaN at 130 and numbers at 1150, the oracle likewise
  planted mistakes on the data the old parity tests use (bench graph 1000 x 200 with its decoys, thr = 1.2, equality with the oracle; the
  first 1500 observations here, all 8000 give the same sets):
      caught there       no_diag, trunc_query, sign_nofabs
      NOT caught there   le (nothing at equality), nearest and type_nofabs (the decoys come AFTER the cones they shadow), no_carry (270
                         cones: one scan pass), overwrite (one tile), count_nonfinite (no such cone), trunc
  every one of them is caught by a case here (`le` by the equality construction alone), except `trunc`, which is harmless by itself —
  truncation in cones and queries alike only widens cells (assoc_exec's docstring) — and is asserted to change no answer anywhere."""
import numpy as np
import pytest

import assoc_exec as ax
import frontend_exact_ref as fx
import frontend_shapes as fs

MP, mpf, U = fx.MP, fx.mpf, fx.U


def rel(a, b):
    """the max-norm measure of test_gpu_parity.py"""
    s = max(np.nanmax(np.abs(b)), 1e-300)
    return np.nanmax(np.abs(a - b)) / s


def frame_exec(c, signed, bugs=()):
    return ax.run("frame", c["poses"], c["pose_of"], c["obs"], c["lidar"], c["map_xy"], c["map_ty"], c["thr"], c["tol"], bugs, signed)


# ---------------------------------------------------------------- the census
def test_the_cases_reach_every_named_edge():
    C = {n: fs.case(n) for n in fs.NAMES}
    # A0: both lidar offsets; the edges
    assert {C[n]["lidar"] for n in fs.NAMES if C[n]["family"].startswith("a0")} == {1.5, 0.0}
    for n in ("a0_edges", "a0_edges_l0"):
        ob = C[n]["obs"]; R = fs.reference(n); l = C[n]["lidar"]
        az, zen, d = ob[:, 0], ob[:, 1], ob[:, 2]
        assert ((az == 0) & ~np.signbit(az)).any() and ((az == 0) & np.signbit(az)).any() and R.nan[az == 0].all()
        assert all(((az == v).any() for v in (180.0, -180.0, 5e-324, -5e-324, 1e-9, -1e-9)))
        assert (zen == 90).any() and (zen == -90).any() and (d == 0).any()
        assert R.nan.sum() == ((az == 0) | ((d == 0) & (l == 0))).sum()
        ok = ~R.nan
        assert (np.sign(R.z_hi[ok, 1]) != np.sign(az[ok])).any(), "no entry where the float kPiF flips the sign of y (az -> 0)"
        if l:
            dnew = np.hypot(R.z_hi[:, 0], R.z_hi[:, 1]) / np.abs(np.cos(zen * ax.K_D2R))
            assert np.nanmin(dnew) < 2e-5, "no entry with dnew -> 0"
    # abeam: the branch band is populated, on both sides of az, and numpy's own NaN falls inside it
    nan_np = 0
    for n in ("a0_abeam", "a0_abeam_l0"):
        c = C[n]; R = fs.reference(n)
        z = ax.polar_to_xy(c["obs"][:, 0], c["obs"][:, 1], c["obs"][:, 2], c["lidar"])
        assert R.band.sum() >= 200 and (c["obs"][R.band, 0] > 0).any() and (c["obs"][R.band, 0] < 0).any()
        assert not np.isnan(z[~R.band]).any() and not R.nan.any()
        nan_np += int(np.isnan(z[R.band]).all(axis=1).sum())
        assert (R.Bz[R.band, 0] > 1e3 * U * np.abs(c["obs"][R.band, 2])).all(), "the bound of x does not widen at the branch point"
        assert len(np.unique(c["obs"][:, 2])) >= (400 if c["lidar"] else 60)
    assert nan_np > 0
    assert not any(fs.reference(n).band.any() for n in fs.NAMES if not n.startswith("a0_abeam"))
    # shapes
    sizes = {len(C[n]["map_xy"]) for n in fs.NAMES}
    assert {0, 1, 255, 256, 257, 1023, 1024, 1025, 2047, 2048} <= sizes
    ns = {len(C[n]["obs"]) for n in fs.NAMES}
    assert {1, 64, 65} <= ns and any(k > 256 and k % 256 for k in ns) and 255 in ns and 257 in ns
    assert all(len(C[n]["poses"]) == 1 for n in ("k1", "k64", "k65", "frame_lanes"))
    for n in ("tile2", "frame_lanes", "type_tol1", "type_tol1p", "grid_crowd", "grid_nonfinite"):
        A = fs.admissible(n)
        for i, j in C[n]["notes"]["expect"].items():
            assert A.mstar[i] == j and i not in A.extra, (n, i, int(A.mstar[i]), j)
        for i, j in C[n]["notes"].get("expect_signed", {}).items():
            assert fs.admissible(n, signed=True).mstar[i] == j, (n, i)
    assert C["type_tol1"]["tol"] == 1.0 and C["type_tol1p"]["tol"] == np.nextafter(1.0, np.inf)
    assert fs.admissible("tile2").mstar[0] == ax.TILE
    # the grid
    cell = lambda n: 1.0 / ax.inv_cell_of(C[n]["thr"])
    assert (C["grid_neg"]["map_xy"] < 0).all() and (fs.reference("grid_neg").g_hi < 0).all()
    c = C["grid_border"]; k = c["map_xy"] / cell("grid_border")
    assert ((k == np.round(k)).sum(axis=0) >= 100).all(), "cones exactly on cell borders, in x and in y"
    c = C["grid_diag"]; A = fs.admissible("grid_diag"); R = fs.reference("grid_diag")
    cq = np.floor(R.g_hi / cell("grid_diag")); cm = np.floor(c["map_xy"][A.mstar] / cell("grid_diag"))
    assert (A.mstar >= 0).all() and (np.abs(cm - cq) == 1).all(), "every query's only match sits in a diagonally adjacent cell"
    c = C["grid_crowd"]; cc = np.floor(c["map_xy"] / cell("grid_crowd")); _, cnt = np.unique(cc, axis=0, return_counts=True)
    assert cnt.max() >= 100
    c = C["km_spread"]; inv = ax.inv_cell_of(c["thr"]); B = ax.buckets_of(len(c["map_xy"]))
    assert B == 8192 and ax.buckets_of(1024) == 4096 and ax.buckets_of(1025) == 8192            # the scan: one pass, and two
    cc = np.stack([ax.grid_coord(c["map_xy"][:, 0], inv), ax.grid_coord(c["map_xy"][:, 1], inv)], axis=1); bk = ax.grid_bucket(cc[:, 0], cc[:, 1], B - 1)
    shared = sum(len(np.unique(cc[bk == b], axis=0)) > 1 for b in np.unique(bk))
    assert shared >= 50, "buckets that hold several far cells"
    assert not np.isfinite(C["grid_nonfinite"]["map_xy"]).all(axis=1)[C["grid_nonfinite"]["notes"]["nonfinite"]].any()
    assert {C[n]["thr"] for n in fs.NAMES if C[n]["thr"] > 0} >= {1e-3, 1.2, 3.0, 1e6}
    assert C["thr_0"]["thr"] == 0 and C["thr_neg"]["thr"] < 0 and np.isnan(C["thr_nan"]["thr"])
    assert all((fs.admissible(n).mstar == -1).all() and not fs.admissible(n).extra for n in ("thr_0", "thr_neg", "thr_nan", "map0"))
    assert (fs.admissible("thr_1e6").mstar >= 0).all()
    # kilometres, and the 3 x 3 guarantee's range
    for n in ("km_spread", "km_neg"):
        assert np.abs(C[n]["poses"][:, :2]).min() > 5.0e3 and np.abs(fs.reference(n).g_hi).max() > 25.0e3
    for n in fs.NAMES:
        xy = C[n]["map_xy"][np.isfinite(C[n]["map_xy"]).all(axis=1)]
        far = max(np.abs(xy).max() if len(xy) else 0.0, np.nanmax(np.abs(fs.reference(n).g_hi)) if len(C[n]["obs"]) else 0.0)
        if C[n]["thr"] > 0:
            assert far / C[n]["thr"] < 4.5e6 / 4, (n, far)
    # near the threshold: 4 .. 16 bands inside and outside, exactly
    c = C["near_thr"]; R = fs.reference("near_thr"); A = fs.admissible("near_thr"); band = R.band_of(c["thr"])
    for i, j, inside in c["notes"]["pairs"]:
        g = [mpf(R.g_hi[i, a]) + mpf(R.g_lo[i, a]) for a in (0, 1)]
        d = MP.sqrt((mpf(c["map_xy"][j, 0]) - g[0]) ** 2 + (mpf(c["map_xy"][j, 1]) - g[1]) ** 2)
        k = float((d - mpf(c["thr"])) / mpf(band[i]))
        assert (-16 < k < -4) if inside else (4 < k < 16), (i, j, k)
        assert (0 <= A.mstar[i] <= j) if inside else (A.mstar[i] != j)
    assert A.n_exact_pairs >= 250 and len(A.extra) >= 20 and all(400 + i in A.extra[i] for i in A.extra), "the in-band branch of the checker is not reached"
    assert not any(fs.admissible(n).extra for n in fs.NAMES if n != "near_thr")


def test_no_random_case_holds_a_candidate_inside_the_band():
    """the cap is zero: what the device answers on a random case is decided outside the band, so its check is an equality"""
    rnd = [n for n in fs.NAMES if fs.case(n)["random"]]
    assert len(rnd) >= 20
    for n in rnd:
        for signed in (False, True):
            A = fs.admissible(n, signed)
            assert A.n_inband == 0 and not A.extra, (n, signed, A.n_inband)


# ---------------------------------------------------------------- numpy and the oracle inside the bound
def test_numpy_and_the_oracle_stay_inside_the_bound_and_the_admissible_sets(po):
    worst = {}; band = dict(numpy=[0, 0], oracle=[0, 0])
    fe = {l: po.OracleFrontend(l) for l in (1.5, 0.0)}
    for n in fs.NAMES:
        c = fs.case(n); R = fs.reference(n); ob = c["obs"]
        paths = dict(numpy=(ax.polar_to_xy(ob[:, 0], ob[:, 1], ob[:, 2], c["lidar"]), ax.cone_to_global(c["poses"], c["pose_of"], ob, c["lidar"])),
                     oracle=(fe[c["lidar"]].polar_to_xy(ob[:, 0], ob[:, 1], ob[:, 2]), fe[c["lidar"]].cone_to_global(c["poses"], c["pose_of"], ob)))
        for who, (z, g) in paths.items():
            sz = fx.check_xy(z, R.z_hi, R.z_lo, R.Bz, R.nan, R.band, (n, who, "z")); sg = fx.check_xy(g, R.g_hi, R.g_lo, R.Bg, R.nan, R.band, (n, who, "g"))
            for k, s in (("z", sz), ("g", sg)):
                worst[who, k] = max(worst.get((who, k), 0.0), s["worst"]); worst[who, k + " band"] = max(worst.get((who, k + " band"), 0.0), s["worst_band"])
            band[who][0] += sz["band_nan"]; band[who][1] += sz["band_num"]
            assert sz["band_nan"] == sg["band_nan"]
        A = fs.admissible(n); As = fs.admissible(n, signed=True)
        gn = np.isnan(paths["oracle"][1]).any(axis=1)
        A.check(fe[c["lidar"]].associate(c["poses"], c["pose_of"], ob, c["map_xy"], c["map_ty"], c["thr"], c["tol"]), gn, (n, "oracle"))
        gn = np.isnan(paths["numpy"][1]).any(axis=1)
        for algo in ("tiled", "grid", "frame"):
            A.check(ax.run(algo, c["poses"], c["pose_of"], ob, c["lidar"], c["map_xy"], c["map_ty"], c["thr"], c["tol"]), gn, (n, algo))
        As.check(frame_exec(c, True), gn, (n, "frame signed"))
    print("worst err / B:", {k: round(v, 3) for k, v in worst.items()}, "branch band NaN / numbers:", band)
    assert max(worst.values()) <= 1.0 and band["numpy"][0] > 0


# ---------------------------------------------------------------- the planted mistakes
ORDER = ("tile2", "frame_lanes", "type_tol1", "type_tol1p", "grid_diag", "grid_nonfinite", "grid_neg", "grid_border", "map1025", "thr_3", "km_spread", "a0_random")


def caught_by(bug, algo):
    for n in ORDER:
        c = fs.case(n)
        got = ax.run(algo, c["poses"], c["pose_of"], c["obs"], c["lidar"], c["map_xy"], c["map_ty"], c["thr"], c["tol"], (bug,))
        gn = np.isnan(ax.cone_to_global(c["poses"], c["pose_of"], c["obs"], c["lidar"], (bug,))).any(axis=1)
        if fs.admissible(n).failures(got, gn):
            return n
    return None


def equality_cases(run):
    """the equality construction on a path `run(obs, map_xy, map_ty, thr) -> idx` with the path's own global XY; returns the failures"""
    g = ax.cone_to_global(fs.EQ_POSE, np.zeros(len(fs.EQ_OBS), dtype=np.int32), fs.EQ_OBS, 1.5)
    assert np.array_equal(g, ax.polar_to_xy(fs.EQ_OBS[:, 0], fs.EQ_OBS[:, 1], fs.EQ_OBS[:, 2], 1.5))       # pose at the origin: gxy IS the A0 output
    bad = []
    for i, xy, ty, thr, j in fs.equality_maps(g):
        want = np.full(len(g), -1); at = run(xy, ty, thr)
        want2 = want.copy(); want2[i] = j; above = run(xy, ty, float(np.nextafter(thr, np.inf)))
        if not (np.array_equal(at, want) and np.array_equal(above, want2)):
            bad.append((i, j))
    return bad


def test_every_planted_mistake_is_caught_by_a_case():
    report = {}
    for bug in ax.ALL_BUGS:
        for algo in ax.APPLIES[bug]:
            report[bug, algo] = caught_by(bug, algo)
    # `<=` for `<` shows only at equality: the bit-for-bit cases
    for algo in ("tiled", "grid", "frame"):
        honest = lambda xy, ty, thr, b=(): ax.run(algo, fs.EQ_POSE, np.zeros(len(fs.EQ_OBS), dtype=np.int32), fs.EQ_OBS, 1.5, xy, ty, thr, 1e-4, b)
        assert not equality_cases(honest), algo
        assert equality_cases(lambda xy, ty, thr: honest(xy, ty, thr, ("le",))), algo
        assert report["le", algo] is None                                     # (no other case can see it: nothing else sits at equality)
        report["le", algo] = "equality"
    print("caught by:", report)
    harmless = {k: v for k, v in report.items() if k[0] == "trunc"}
    assert all(v is None for v in harmless.values())
    for n in [n for n in fs.NAMES if fs.case(n)["thr"] > 0 and len(fs.case(n)["map_xy"])]:          # truncation on both sides changes no answer anywhere
        c = fs.case(n); g = ax.cone_to_global(c["poses"], c["pose_of"], c["obs"], c["lidar"])
        assert np.array_equal(ax.grid(g, c["obs"][:, 3], c["map_xy"], c["map_ty"], c["thr"], c["tol"], ("trunc",)),
                              ax.grid(g, c["obs"][:, 3], c["map_xy"], c["map_ty"], c["thr"], c["tol"])), n
    missed = [k for k, v in report.items() if v is None and k[0] != "trunc"]
    assert not missed, missed


OLD_DATA_CATCHES = {"no_diag", "trunc_query", "sign_nofabs"}


def test_what_the_old_parity_data_catches_of_the_planted_mistakes(pkg, frontend, bench_graphs):
    """test_association_fixed_map_bit_exact's data (bench graph 1000 x 200, decoys, thr = 1.2): a planted result that EQUALS the oracle's
    there would have passed the old suite"""
    t, g = bench_graphs(1000, 200)
    N, K = len(t["odom_poses"]), t["K"]
    obs = t["obs"].reshape(-1, 4)[:1500]; po_ = np.repeat(np.arange(N, dtype=np.int32), K)[:1500]
    map_xy = np.concatenate([t["cone_xy"][g["map_true_id"]], t["cone_xy"][g["map_true_id"]][:20] + 0.05])
    map_type = np.concatenate([g["lm_type"], (g["lm_type"][:20] % 4) + 1]).astype(np.int32)
    ref = frontend.associate(t["truth_poses"], po_, obs, map_xy, map_type, 1.2)
    caught = set()
    for bug in ax.ALL_BUGS:
        for algo in ax.APPLIES[bug]:
            got = ax.run(algo, t["truth_poses"], po_, obs, 1.5, map_xy, map_type, 1.2, 1e-4, (bug,))
            if not np.array_equal(got, ref):
                caught.add(bug)
    for algo in ("tiled", "grid", "frame"):
        assert np.array_equal(ax.run(algo, t["truth_poses"], po_, obs, 1.5, map_xy, map_type, 1.2, 1e-4), ref)
    print("the old data catches:", sorted(caught), "and misses:", sorted(set(ax.ALL_BUGS) - caught))
    assert caught == OLD_DATA_CATCHES


# ---------------------------------------------------------------- the bound against the max-norm
def test_perturbations_that_the_max_norm_passes_are_refused_by_the_bound():
    c = fs.case("a0_abeam"); R = fs.reference("a0_abeam"); ob = c["obs"]
    z = ax.polar_to_xy(ob[:, 0], ob[:, 1], ob[:, 2], 1.5)
    fx.check_xy(z, R.z_hi, R.z_lo, R.Bz, R.nan, R.band)
    i = int(np.flatnonzero(R.band & ~np.isnan(z).any(axis=1))[0])                # y of an abeam entry: the asin error does not reach it to first order
    p = z.copy(); p[i, 1] += 4 * R.Bz[i, 1]
    assert 4 * R.Bz[i, 1] < 1e3 * U * abs(z[i, 1]) and rel(p, z) < 1e-12
    with pytest.raises(AssertionError):
        fx.check_xy(p, R.z_hi, R.z_lo, R.Bz, R.nan, R.band)
    c = fs.case("a0_edges"); R = fs.reference("a0_edges"); ob = c["obs"]
    z = ax.polar_to_xy(ob[:, 0], ob[:, 1], ob[:, 2], 1.5)
    i = int(np.flatnonzero((ob[:, 0] == 1e-9) & (ob[:, 2] == 7.0) & (ob[:, 1] == 0.0))[0])       # a small y next to the array's largest entry
    p = z.copy(); p[i, 1] += 4 * R.Bz[i, 1]
    assert abs(z[i, 1]) < 1e-6 and rel(p, z) < 1e-12
    with pytest.raises(AssertionError):
        fx.check_xy(p, R.z_hi, R.z_lo, R.Bz, R.nan, R.band)
    # the double pi in place of the float kPiF passes nothing
    c = fs.case("a0_random"); R = fs.reference("a0_random"); ob = c["obs"]
    old = ax.K_PIF
    try:
        ax.K_PIF = float(np.pi); zpi = ax.polar_to_xy(ob[:, 0], ob[:, 1], ob[:, 2], 1.5)
    finally:
        ax.K_PIF = old
    with pytest.raises(AssertionError):
        fx.check_xy(zpi, R.z_hi, R.z_lo, R.Bz, R.nan, R.band)
