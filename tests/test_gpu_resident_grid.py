"""GPU test of the resident map's grid cache (gs_frontend.cpp, resident_map / map_changed): one handle with the hashed grid forced, three
frames of 8, 13 and 20 observations, and the resident map taken through every call that changes it.  At every step
gs_associate_nn_resident, gs_assign_opt_resident and gs_relocalize_resident run against the resident map, and every output array must equal,
byte for byte, what the matching _batch call returns for the same map arrays and options — a batch call stages its map and builds its grid
from nothing on every call, so it cannot be stale.  (Both sides are held to the numpy references by the suites of their own.)  A grid that
was not rebuilt after a map change still returns plausible indices; only this comparison shows it.  After every step one of the three
calls is repeated unchanged and must return the same bytes: the path that finds its grid valid.

The scene: three frontend_shapes scenes of one pose each, 1 500 cones each, a cone planted 5 cm from every observation (so that the
association matches and the relocalisation finds the frame), interleaved so that the first 300 cones hold the first 100 of each.
300 cones take 4 096 buckets, 4 500 take 32 768: the append makes the grid's allocation grow; the 40 cones at the end sit inside it."""
import numpy as np
import pytest

import frontend_shapes as fs

pytestmark = pytest.mark.gpu
SIZES = (8, 13, 20)
CENTRES = ((0.0, 0.0), (150.0, 40.0), (-120.0, 90.0))
HEAD = 100                                                     # cones of each scene among the first 300


def build_scene():
    parts = []
    for f, (k, centre) in enumerate(zip(SIZES, CENTRES)):
        c = fs.scene(900 + f, k, 1500, centre=centre, n_poses=1, attach=0.3)
        for i in range(k):
            a = 0.7 * i + f
            fs.plant(c, i, i, (0.04 * np.cos(a), 0.04 * np.sin(a)))          # cone i: 0.04 thr = 4.8 cm from observation i, its type
        parts.append(c)
    xy = np.concatenate([c["map_xy"][:HEAD] for c in parts] + [c["map_xy"][HEAD:] for c in parts])
    ty = np.concatenate([c["map_ty"][:HEAD] for c in parts] + [c["map_ty"][HEAD:] for c in parts]).astype(np.int32)
    poses = np.concatenate([c["poses"] for c in parts]); obs = np.concatenate([c["obs"] for c in parts])
    pose_of = np.repeat(np.arange(3), SIZES).astype(np.int32); frame_start = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    return poses, pose_of, obs, frame_start, np.ascontiguousarray(xy), np.ascontiguousarray(ty)


def same_bytes(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class Resident:
    """the frames in device memory, an output buffer per array of the three resident calls, and the calls"""
    RELOC = (("pose", np.float64, 3), ("count", np.int32, 1), ("cost", np.float64, 1), ("seed", np.int32, 4), ("second_count", np.int32, 1),
             ("second_pose", np.float64, 3), ("n_seeds", np.int64, 1), ("status", np.int32, 1))

    def __init__(self, pkg, G, poses, pose_of, obs, frame_start):
        DA = pkg.binding.DeviceArray
        self.G = G; self.n = len(obs); self.nf = len(frame_start) - 1; self.np = len(poses)
        self.p, self.po, self.ob, self.fs = DA(np.ascontiguousarray(poses)), DA(pose_of), DA(np.ascontiguousarray(obs)), DA(frame_start)
        self.i32 = [DA(nbytes=4 * self.n) for _ in range(3)]; self.f64 = [DA(nbytes=8 * self.n) for _ in range(2)]
        self.rl = {name: DA(nbytes=np.dtype(t).itemsize * w * self.nf) for name, t, w in self.RELOC}
        self.all = [self.p, self.po, self.ob, self.fs] + self.i32 + self.f64 + list(self.rl.values())

    def nn(self, nnp, rlp):
        self.G.associate_nn_resident(self.p, self.np, self.po, self.ob, self.n, self.i32[0], self.f64[0], self.f64[1], params=nnp); self.G.synchronize()
        return self.i32[0].to_host(np.int32, self.n), self.f64[0].to_host(np.float64, self.n), self.f64[1].to_host(np.float64, self.n)

    def assign(self, nnp, rlp):
        self.G.assign_opt_resident(self.p, self.np, self.po, self.ob, self.n, self.nf, self.fs, self.i32[0], self.f64[0], self.i32[1], params=nnp); self.G.synchronize()
        return self.i32[0].to_host(np.int32, self.n), self.f64[0].to_host(np.float64, self.n), self.i32[1].to_host(np.int32, self.n)

    def reloc(self, nnp, rlp):
        r = self.rl
        self.G.relocalize_resident(self.ob, self.n, self.nf, self.fs, r["pose"], r["count"], r["cost"], r["seed"], r["second_count"], r["second_pose"], r["n_seeds"],
                                   r["status"], self.i32[2], self.f64[1], params=rlp); self.G.synchronize()
        rec = {name: r[name].to_host(t, w * self.nf).reshape((self.nf, w) if w > 1 else (self.nf,)) for name, t, w in self.RELOC}
        return rec, self.i32[2].to_host(np.int32, self.n), self.f64[1].to_host(np.float64, self.n)

    def free(self):
        for a in self.all:
            a.free()


def flat(res):
    """a call's outputs as a list of (name, array)"""
    out = []
    for k, r in enumerate(res):
        out += [(name, r[name]) for name in sorted(r)] if isinstance(r, dict) else [("out%d" % k, r)]
    return out


def test_resident_calls_equal_the_batch_calls_through_every_map_change(pkg):
    if pkg.device_count() < 1:
        pytest.fail("no gfx950 device visible: the HIP path cannot run")
    B = pkg.binding
    poses, pose_of, obs, frame_start, xy, ty = build_scene()
    assert len(ty) == 4500 and tuple(np.diff(frame_start)) == SIZES
    G = pkg.Graph(); G.set_debug(assoc_grid=1)
    D = Resident(pkg, G, poses, pose_of, obs, frame_start)
    calls = (("associate_nn", D.nn), ("assign_opt", D.assign), ("relocalize", D.reloc))
    turn = [0]; matched = []

    def held(tag, mxy, mty, nnp, rlp):
        """the three resident calls against the batch calls on (mxy, mty); then one of them again, on the grid it left behind"""
        assert G.map_size() == len(mty), (tag, G.map_size(), len(mty))
        want = {"associate_nn": G.associate_nn(poses, pose_of, obs, mxy, mty, params=nnp),
                "assign_opt": G.assign_opt(poses, pose_of, obs, frame_start, mxy, mty, params=nnp),
                "relocalize": G.relocalize(obs, frame_start, mxy, mty, params=rlp)}
        again = calls[turn[0] % 3]; turn[0] += 1
        for name, call in calls + (again,):
            for (field, w), (_, got) in zip(flat(want[name]), flat(call(nnp, rlp))):
                assert same_bytes(got, w), (tag, name, field, "resident differs from batch", int((np.asarray(got) != np.asarray(w)).sum()))
        matched.append((tag, int((want["associate_nn"][0] >= 0).sum()), int((want["assign_opt"][0] >= 0).sum()), want["relocalize"][0]["status"].tolist()))
        return want

    nn_a, nn_b = B.nn_params(), B.nn_params(max_distance=2.0)
    rl_a, rl_b = B.reloc_params(), B.reloc_params(inlier_radius=0.8)
    # (a) 300 cones: 4 096 buckets
    G.map_append(xy[:300], ty[:300])
    held("a: 300 cones", xy[:300], ty[:300], nn_a, rl_a)
    # (b) appended to 4 500: 32 768 buckets, both grids' allocations grow
    G.map_append(xy[300:], ty[300:])
    held("b: 4500 cones", xy, ty, nn_a, rl_a)
    # (c) each distance changed by itself, and back: a call rebuilds its own grid, the other call's stays what it was
    held("c: max_distance 2.0", xy, ty, nn_b, rl_a)
    held("c: max_distance back", xy, ty, nn_a, rl_a)
    held("c: inlier_radius 0.8", xy, ty, nn_a, rl_b)
    wc = held("c: both changed", xy, ty, nn_b, rl_b)
    # (d) ten planted cones (all eight of the first frame, two of the second) moved by more than either cell edge (2.0, 0.8)
    moved = xy.copy()
    moved[:8] += (7.0, -6.0); moved[HEAD:HEAD + 2] += (-9.0, 5.0)
    G.map_set_xy(0, moved[:8]); G.map_set_xy(HEAD, moved[HEAD:HEAD + 2])
    wd = held("d: set_xy", moved, ty, nn_b, rl_b)
    assert not same_bytes(wd["associate_nn"][0], wc["associate_nn"][0]) and not same_bytes(wd["relocalize"][0]["pose"], wc["relocalize"][0]["pose"]), "the move shows in the results"
    held("d: set_xy, first distances", moved, ty, nn_a, rl_a)
    # (e) five planted twins appended, then merged away in the resident map
    twins = np.array([2 * HEAD, 2 * HEAD + 1, 2 * HEAD + 2, HEAD + 5, HEAD + 6])
    txy = np.concatenate([moved, moved[twins] + 0.01]); tty = np.concatenate([ty, ty[twins]])
    G.map_append(txy[4500:], tty[4500:])
    held("e: twins appended", txy, tty, nn_a, rl_a)
    mxy, mty, _, _, binfo = G.map_merge_twins_batch(txy, tty)
    _, info = G.map_merge_twins()
    assert int(info["n_pairs"]) >= 5 and int(info["n_out"]) == len(mty) <= 4500 and int(info["n_pairs"]) == int(binfo["n_pairs"])
    rxy, rty = G.map_xy()
    assert same_bytes(rxy, mxy) and same_bytes(rty, mty), "the resident merge and the batch merge leave the same map"
    held("e: twins merged", mxy, mty, nn_a, rl_a)
    # (f) cleared, then 40 cones inside the larger allocation
    G.map_clear()
    G.map_append(xy[:40], ty[:40])
    held("f: 40 cones", xy[:40], ty[:40], nn_a, rl_a)
    held("f: 40 cones, other distances", xy[:40], ty[:40], nn_b, rl_b)
    for m in matched:
        print("%-32s associate_nn matched %2d, assign_opt matched %2d, relocalize status %s" % m)
    assert matched[0][1] >= 30 and 0 in matched[1][3], "the scene exercises the search: most observations match, a frame is found on the map"
    D.free(); G.close()
