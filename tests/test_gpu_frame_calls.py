"""GPU test of what the live frame calls (gs_frame_frontend*) share on a handle: their pinned / device staging and the one chain run.

One map of 48 cones with covariances.  A long-lived handle runs frames of 1, 65, 0, 256, 64, 98 and 97 observations, in this order — the staging
grows (1: room for 64, 65: for 97, 98: for 147, 256), and smaller frames follow larger ones in buffers that still hold the larger frames'
bytes; at k = 1 relocalisation finds no seed.  At every k it runs every live entry point, and every array and record it returns must equal, bit
for bit, the same call on a second handle created for that k alone, which runs the entry points in reverse order.  Once with the whole-map
search and once with the hashed grid; and a call the library refuses (257 observations) leaves the next call's results as they would have been.
The per-stage files hold each call to its batch and resident forms; this one holds the calls to each other's leftovers."""
import numpy as np
import pytest

import assoc_nn_shapes as ns

pytestmark = pytest.mark.gpu
ORDER = (1, 65, 0, 256, 64, 98, 97)
CALLS = ("frame_frontend", "frame_frontend_nn", "frame_frontend_assign", "frame_frontend_assign_opt", "frame_frontend_jc", "frame_frontend_localize",
         "frame_frontend_relocalize", "follow")


@pytest.fixture(scope="module")
def scene():
    """257 observations from one pose, the first 48 of them (for the most part) with a cone of their own among the map's 48"""
    return ns.scene(20260, 257, 48, n_poses=1, spread=30.0)


def raw(x):
    """a result's bytes, NaN-proof: arrays, records (dicts of arrays), numbers, nested in tuples"""
    if isinstance(x, dict):
        return tuple((k, raw(x[k])) for k in sorted(x))
    if isinstance(x, (tuple, list)):
        return tuple(raw(v) for v in x)
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    return x


def handle(pkg, sc, grid):
    g = pkg.Graph(lidar_to_cog=sc["lidar"], debug=dict(assoc_grid=grid))
    g.map_append(sc["map_xy"], sc["map_ty"]); g.map_set_cov(0, sc["map_cov"])
    return g


def call(g, name, sc, k):
    pose, cov, obs = sc["poses"][0], sc["pose_cov"][0], sc["obs"][:k]
    if name == "frame_frontend":
        return g.frame_frontend(pose, obs, 2.0)
    if name == "frame_frontend_relocalize":
        return g.frame_frontend_relocalize(obs, 1.0, 0.2)
    if name == "follow":                                            # two hypotheses, the first frame without a motion, the second with one
        g.follow_set(np.stack([pose, pose + [0.4, -0.3, 0.05]]), np.stack([cov, cov]))
        return g.frame_frontend_follow(obs), g.frame_frontend_follow(obs, [0.05, -0.02, 0.01], np.diag([1e-3, 1e-3, 1e-4]).reshape(9)), g.follow_get()
    return getattr(g, name)(pose, obs, cov)


def every_call(g, sc, k, names):
    return {name: raw(call(g, name, sc, k)) for name in names}


@pytest.mark.parametrize("grid", [0, 1])
def test_a_long_lived_handle_returns_what_a_fresh_one_does(pkg, scene, grid):
    if pkg.device_count() < 1:
        pytest.fail("no gfx950 device visible: the HIP path cannot run")
    sc = scene; H = handle(pkg, sc, grid)
    try:
        for k in ORDER:
            got = every_call(H, sc, k, CALLS)
            F = handle(pkg, sc, grid)
            try:
                want = every_call(F, sc, k, CALLS[::-1])
            finally:
                F.close()
            for name in CALLS:
                assert got[name] == want[name], "k = %d, grid %d: %s on the long-lived handle differs from a fresh handle's" % (k, grid, name)
            if k == 1:                                              # (the no-seed record came from the device, and the chain behind it found an empty frame)
                sr = call(H, "frame_frontend_relocalize", sc, 1)[0]
                assert int(sr["status"][0]) == 2 and int(sr["count"][0]) == 0 and np.isinf(sr["cost"][0]) and (sr["seed"] == -1).all()
        # a refused call leaves nothing behind: the next call on H still equals the fresh handle's
        pose, cov = sc["poses"][0], sc["pose_cov"][0]
        for name in ("frame_frontend_assign", "frame_frontend_assign_opt", "frame_frontend_jc", "frame_frontend_localize"):
            with pytest.raises(pkg.binding.GsError) as e:
                getattr(H, name)(pose, sc["obs"][:257], cov)
            assert e.value.code == -1, e.value                      # GS_ERR_INVALID
        with pytest.raises(pkg.binding.GsError) as e:
            H.frame_frontend_relocalize(sc["obs"][:257], 1.0, 0.2)
        assert e.value.code == -1, e.value
        got = every_call(H, sc, 97, CALLS)
        F = handle(pkg, sc, grid)
        try:
            want = every_call(F, sc, 97, CALLS[::-1])
        finally:
            F.close()
        for name in CALLS:
            assert got[name] == want[name], "after a refused call, grid %d: %s differs from a fresh handle's" % (grid, name)
    finally:
        H.close()
