"""GPU tests of the front end (A0, A1) against the exact reference of tests/frontend_exact_ref.py, on every path and every case of
tests/frontend_shapes.py (test_frontend_exact_cpu.py holds the census of what each case reaches and shows that the checks have teeth).

Every case runs through gs_polar_to_xy_batch, gs_cone_to_global_batch, gs_associate_batch with assoc_grid 0, 1 and -1,
gs_associate_resident with the grid and with brute force, and gs_frame_frontend (per pose) with signed_type 0 and 1:
    A0   every entry of the CoG-frame and the global XY within its bound B (the rounding count is in frontend_exact_ref's docstring); in the
         asin's branch band NaN in both coordinates or a number inside B, nowhere else a NaN the formula does not have
    A1   every index in the query's admissible set: the lowest exact match outside the band, or an in-band index below it; -1 for a NaN query
    the five batch and resident results agree bit for bit (also inside the band); the frame path is held to the checker, and whether its
    out_zxy / out_gxy bits equal the batch outputs is recorded, not asserted
Equality with the threshold is asserted bit for bit on every path from the path's OWN reported global XY (frontend_shapes.equality_maps),
the resident map's state through clear / append / set_xy / capacity growth / threshold changes against the reference on the map as it
should then be.

Measured on an MI355X (profiles/frontend_gpu_suite.txt has every case), worst |got - exact| / B per kernel and case family; the bound comes
from the rounding count alone and was not fitted to these:
  family      k_polar_to_xy   k_cone_to_global   k_frame_frontend z / g
  a0_random        0.270            0.091             0.270 / 0.091
  a0_abeam         0.141            0.141             0.141 / 0.141     outside the branch band
                   0.338            0.338             0.338 / 0.338     inside it, where a number came back
  a0_edges         0.204            0.491             0.204 / 0.491
  shape            0.251            0.128             0.251 / 0.128
  grid             0.217            0.323             0.217 / 0.323
  km               0.205            0.322             0.205 / 0.322
  thr              0.205            0.137             0.205 / 0.137
  near_thr         0.154            0.097             0.154 / 0.097
Branch band (1 280 entries of a0_abeam and a0_abeam_l0): NaN at 126, numbers at 1 154, on every kernel alike (numpy and the CPU
oracle: NaN at 130) — the abeam behaviour of the reference's formula is real on the device: NaN, or an error of order sqrt(u) dist in x.
Every index of every path lay in its admissible set; the five batch and resident results agreed bit for bit on every case, in-band cones
included.  The frame path: out_zxy has the batch path's bits on every case; out_gxy differs from gs_cone_to_global_batch in the last place
on 33 of 37 cases (k_frame_frontend takes cos and sin separately, every other path sincos; the bits are equal with the pose at the origin, on the
two kilometre cases and on the two single-observation cases); its indices equal the batch path's on every case but near_thr, where cones were PLACED inside the band — there
"same arithmetic => identical indices" does not hold for the frame kernel, and cannot be asked of it: both answers are admissible.
Nothing under csrc/ needed a change.
"""
import numpy as np
import pytest

import frontend_exact_ref as fx
import frontend_shapes as fs

pytestmark = pytest.mark.gpu
STATS = {}


@pytest.fixture(scope="module")
def handles(pkg):
    if pkg.device_count() < 1:
        pytest.fail("no gfx950 device visible: the HIP path cannot run")
    H = {1.5: pkg.Graph(), 0.0: pkg.Graph(lidar_to_cog=0.0)}
    yield H
    for g in H.values():
        g.close()


class Dev:
    """a case's poses, pose indices and observations in device memory, with a result buffer"""

    def __init__(self, pkg, poses, pose_of, obs):
        DA = pkg.binding.DeviceArray
        self.n = len(obs); self.np = len(poses)
        self.p, self.po, self.ob, self.out = DA(np.ascontiguousarray(poses, dtype=np.float64)), DA(np.ascontiguousarray(pose_of, dtype=np.int32)), DA(np.ascontiguousarray(obs, dtype=np.float64)), DA(nbytes=4 * self.n)

    def resident(self, G, thr, tol):
        G.associate_resident(self.p, self.np, self.po, self.ob, self.n, thr, self.out, tol); G.synchronize()
        return self.out.to_host(np.int32, self.n)

    def free(self):
        for a in (self.p, self.po, self.ob, self.out):
            a.free()


def set_map(G, xy, ty):
    G.map_clear()
    if len(ty):
        G.map_append(xy, ty)
    assert G.map_size() == len(ty)


def batch_and_resident(pkg, G, poses, pose_of, obs, map_xy, map_ty, thr, tol):
    """the five results of the batch and the resident association: {path: idx}"""
    out = {}
    for mode in (0, 1, -1):
        G.set_debug(assoc_grid=mode)
        out["batch grid=%d" % mode] = G.associate(poses, pose_of, obs, map_xy, map_ty, thr, tol)
    set_map(G, map_xy, map_ty)
    d = Dev(pkg, poses, pose_of, obs)
    out["resident grid"] = d.resident(G, thr, tol)
    G.set_debug(assoc_grid=0)
    out["resident brute"] = d.resident(G, thr, tol)
    G.set_debug(assoc_grid=-1)
    d.free()
    return out


def frame_path(G, poses, pose_of, obs, thr, tol, signed):
    """gs_frame_frontend pose by pose against the resident map, put back in the case's order: z, g, idx"""
    n = len(obs); z = np.zeros((n, 2)); g = np.zeros((n, 2)); idx = np.zeros(n, dtype=np.int32)
    for p in range(len(poses)):
        sel = np.flatnonzero(np.asarray(pose_of) == p)
        if len(sel):
            z[sel], g[sel], idx[sel] = G.frame_frontend(poses[p], obs[sel], thr, tol, signed)
    return z, g, idx


@pytest.mark.parametrize("name", fs.NAMES)
def test_every_path_entry_by_entry(pkg, handles, name):
    c = fs.case(name); R = fs.reference(name); A = fs.admissible(name); As = fs.admissible(name, signed=True)
    G = handles[c["lidar"]]; ob = c["obs"]; args = (c["poses"], c["pose_of"], ob)
    z = G.polar_to_xy(ob[:, 0], ob[:, 1], ob[:, 2]); g = G.cone_to_global(*args)
    st = dict(k_polar_to_xy=fx.check_xy(z, R.z_hi, R.z_lo, R.Bz, R.nan, R.band, (name, "polar_to_xy")),
              k_cone_to_global=fx.check_xy(g, R.g_hi, R.g_lo, R.Bg, R.nan, R.band, (name, "cone_to_global")))
    assert np.array_equal(np.isnan(z), np.isnan(g))
    gn = np.isnan(g).any(axis=1)
    res = batch_and_resident(pkg, G, *args, c["map_xy"], c["map_ty"], c["thr"], c["tol"])
    for path, idx in res.items():
        A.check(idx, gn, (name, path))
    first = res["batch grid=0"]
    assert all(np.array_equal(first, idx) for idx in res.values()), (name, "the batch and resident paths disagree", {k: int((v != first).sum()) for k, v in res.items()})
    zf, gf, i0 = frame_path(G, *args, c["thr"], c["tol"], 0)
    st["k_frame_frontend z"] = fx.check_xy(zf, R.z_hi, R.z_lo, R.Bz, R.nan, R.band, (name, "frame z"))
    st["k_frame_frontend g"] = fx.check_xy(gf, R.g_hi, R.g_lo, R.Bg, R.nan, R.band, (name, "frame g"))
    gfn = np.isnan(gf).any(axis=1)
    A.check(i0, gfn, (name, "frame"))
    zs, gs, i1 = frame_path(G, *args, c["thr"], c["tol"], 1)
    As.check(i1, gfn, (name, "frame signed"))
    assert np.array_equal(zs, zf, equal_nan=True) and np.array_equal(gs, gf, equal_nan=True)
    for i, j in c["notes"].get("expect", {}).items():
        assert first[i] == j and i0[i] == j, (name, i, int(first[i]), int(i0[i]), j)
    for i, j in c["notes"].get("expect_signed", {}).items():
        assert i1[i] == j, (name, i, int(i1[i]), j)
    if not c["thr"] > 0:
        assert (first == -1).all() and (i0 == -1).all() and (i1 == -1).all()
    same = dict(z=bool(np.array_equal(zf, z, equal_nan=True)), g=bool(np.array_equal(gf, g, equal_nan=True)), idx=bool(np.array_equal(i0, first)))
    STATS[name] = (c["family"], st, same)
    print("%-15s %-10s" % (name, c["family"]) + " ".join("| %s %.3f band %.3f nan/num %d/%d " % (k, v["worst"], v["worst_band"], v["band_nan"], v["band_num"]) for k, v in st.items())
          + "| frame bits equal batch: z %(z)s g %(g)s idx %(idx)s" % same)
    G.map_clear()


def test_equality_with_the_threshold_bit_for_bit_on_every_path(pkg, handles):
    """pose at the origin with heading 0, a cone of the query's type at m = fl(g + a) along one axis, thr = m - g: sqrt(dx * dx + 0) == thr
    exactly, so `<` gives no match at thr and a match at the next fp64 above — in x and in y, in a map of two cones and as the first cone of
    the second LDS tile, from each path's own reported global XY"""
    G = handles[1.5]; po_ = np.zeros(len(fs.EQ_OBS), dtype=np.int32); args = (fs.EQ_POSE, po_, fs.EQ_OBS)
    g_batch = G.cone_to_global(*args)
    G.map_clear(); _, g_frame, _ = G.frame_frontend(fs.EQ_POSE[0], fs.EQ_OBS, 1.2)
    assert np.array_equal(g_batch, G.polar_to_xy(fs.EQ_OBS[:, 0], fs.EQ_OBS[:, 1], fs.EQ_OBS[:, 2]))      # the pose at the origin adds nothing
    print("equality: the frame path's global XY bits equal the batch path's:", bool(np.array_equal(g_batch, g_frame)))
    n = 0
    for i, xy, ty, thr, j in fs.equality_maps(g_batch):
        want = np.full(len(po_), -1); hit = want.copy(); hit[i] = j
        for t, w in ((thr, want), (float(np.nextafter(thr, np.inf)), hit)):
            for path, idx in batch_and_resident(pkg, G, *args, xy, ty, t, 1e-4).items():
                assert np.array_equal(idx, w), (path, i, j, t, idx.tolist()); n += 1
    for i, xy, ty, thr, j in fs.equality_maps(g_frame):
        want = np.full(len(po_), -1); hit = want.copy(); hit[i] = j
        set_map(G, xy, ty)
        for t, w in ((thr, want), (float(np.nextafter(thr, np.inf)), hit)):
            for signed in (0, 1):
                _, gf, idx = G.frame_frontend(fs.EQ_POSE[0], fs.EQ_OBS, t, 1e-4, signed)
                assert np.array_equal(gf, g_frame) and np.array_equal(idx, w), ("frame", signed, i, j, t, idx.tolist()); n += 1
    assert n == 16 * 2 * 5 + 16 * 2 * 2
    G.map_clear()


def held(pkg, G, c, R, map_xy, map_ty, thr, tag):
    """the resident map as it should now be: both resident kernels and the frame path against the reference on (map_xy, map_ty)"""
    A = R.admissible(map_xy, map_ty, thr, c["tol"]); As = R.admissible(map_xy, map_ty, thr, c["tol"], signed=True)
    assert G.map_size() == len(map_ty), (tag, G.map_size(), len(map_ty))
    d = Dev(pkg, c["poses"], c["pose_of"], c["obs"])
    G.set_debug(assoc_grid=-1); a = d.resident(G, thr, c["tol"])
    G.set_debug(assoc_grid=0); b = d.resident(G, thr, c["tol"]); G.set_debug(assoc_grid=-1)
    d.free()
    A.check(a, None, (tag, "resident grid")); assert np.array_equal(a, b), (tag, "grid and brute force disagree")
    _, gf, i0 = frame_path(G, c["poses"], c["pose_of"], c["obs"], thr, c["tol"], 0)
    A.check(i0, np.isnan(gf).any(axis=1), (tag, "frame"))
    As.check(frame_path(G, c["poses"], c["pose_of"], c["obs"], thr, c["tol"], 1)[2], np.isnan(gf).any(axis=1), (tag, "frame signed"))
    return a


def test_the_resident_map_through_its_state_changes(pkg):
    """clear then re-append the same count (the grid cache is keyed on the count and the threshold), a partial set_xy, two appends with no
    frame between them (the wait on the pinned staging buffer), an append across the 1024-cone capacity (the old cones are copied device to
    device), a threshold change and back, and a set_xy beyond the end (refused, nothing changes)"""
    c = fs.case("map2048"); R = fs.reference("map2048"); xy, ty = c["map_xy"], c["map_ty"]; thr = c["thr"]
    G = pkg.Graph()
    G.map_append(xy[:300], ty[:300])
    first = held(pkg, G, c, R, xy[:300], ty[:300], thr, "300 cones")
    G.map_clear(); G.map_append(xy[300:600], ty[300:600])                             # the same count, other cones
    again = held(pkg, G, c, R, xy[300:600], ty[300:600], thr, "cleared, 300 other cones")
    assert not np.array_equal(first, again)
    G.map_append(xy[600:700], ty[600:700]); G.map_append(xy[700:1000], ty[700:1000])  # back to back
    cur_xy = xy[300:1000].copy(); cur_ty = ty[300:1000].copy()
    held(pkg, G, c, R, cur_xy, cur_ty, thr, "two appends")
    moved = xy[:150] + [0.4, -0.3]
    G.map_set_xy(200, moved); cur_xy[200:350] = moved                                 # first > 0
    after = held(pkg, G, c, R, cur_xy, cur_ty, thr, "partial set_xy")
    with pytest.raises(pkg.binding.GsError) as e:
        G.map_set_xy(600, xy[:101])                                                   # 600 + 101 > 700
    assert e.value.code == -1 and G.map_size() == 700
    with pytest.raises(pkg.binding.GsError):
        G.map_set_xy(701, xy[:1])
    assert np.array_equal(held(pkg, G, c, R, cur_xy, cur_ty, thr, "refused set_xy"), after)
    G.map_append(xy[1000:1400], ty[1000:1400])                                        # 700 -> 1100: across the 1024-cone capacity
    cur_xy = np.concatenate([cur_xy, xy[1000:1400]]); cur_ty = np.concatenate([cur_ty, ty[1000:1400]])
    at12 = held(pkg, G, c, R, cur_xy, cur_ty, thr, "across the capacity")
    at3 = held(pkg, G, c, R, cur_xy, cur_ty, 3.0, "thr 3.0")
    assert not np.array_equal(at12, at3)
    assert np.array_equal(held(pkg, G, c, R, cur_xy, cur_ty, thr, "thr back"), at12)
    G.map_append(xy[1400:], ty[1400:]); G.map_append(xy[:300], ty[:300])              # a second growth (1100 -> 2048), again back to back
    held(pkg, G, c, R, np.concatenate([cur_xy, xy[1400:], xy[:300]]), np.concatenate([cur_ty, ty[1400:], ty[:300]]), thr, "grown twice")
    G.close()


def test_the_frame_staging_buffers_grow_at_65_observations(pkg):
    """a fresh handle: k = 1, 64 (the first capacity), 65 (it grows), then 1 again, each against the reference"""
    G = pkg.Graph()
    for name in ("k1", "k64", "k65", "k1"):
        c = fs.case(name); R = fs.reference(name); A = fs.admissible(name)
        set_map(G, c["map_xy"], c["map_ty"])
        z, g, idx = G.frame_frontend(c["poses"][0], c["obs"], c["thr"], c["tol"])
        fx.check_xy(z, R.z_hi, R.z_lo, R.Bz, R.nan, R.band, name); fx.check_xy(g, R.g_hi, R.g_lo, R.Bg, R.nan, R.band, name)
        A.check(idx, np.isnan(g).any(axis=1), name)
    G.close()


def test_zz_the_record_of_what_was_measured():
    """prints, per kernel and case family, the worst err / B of the cases that ran in this session (profiles/frontend_gpu_suite.txt)"""
    fam = {}
    for name, (family, st, same) in STATS.items():
        for k, v in st.items():
            f = fam.setdefault((family, k), dict(worst=0.0, worst_band=0.0, band_nan=0, band_num=0))
            f["worst"] = max(f["worst"], v["worst"]); f["worst_band"] = max(f["worst_band"], v["worst_band"]); f["band_nan"] += v["band_nan"]; f["band_num"] += v["band_num"]
    for (family, k), f in sorted(fam.items()):
        print("RECORD %-10s %-20s worst %.3f  in band (numbers) %.3f  band NaN %d  band numbers %d" % (family, k, f["worst"], f["worst_band"], f["band_nan"], f["band_num"]))
    print("RECORD frame bits equal batch on every case: z %s g %s idx %s" % tuple(all(s[2][k] for s in STATS.values()) for k in ("z", "g", "idx")))
    print("RECORD frame bits differ on:", sorted(n for n, s in STATS.items() if not (s[2]["z"] and s[2]["g"])))
