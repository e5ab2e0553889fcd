"""GPU tests of the time_* twins of the resident front-end calls: a twin repeats the resident call `reps` times between events, so it must be
handed exactly the resident call's arguments.  Per family: the resident call on output buffers filled with a pattern, then the twin on
fresh buffers of the same pattern with every optional output given; the twin returns finite, positive milliseconds and leaves every buffer
byte for byte as the resident call left it.  time_map_merge_twins leaves the resident map as it was.

One scene serves all families, the smallest that reaches every branch of the argument builders: a map of 8 cones with covariances (two of
them twins), one pose with a covariance, two frames of 3 and 0 observations, reps = 2; for follow and cand 2 hypotheses and 2 steps."""
import numpy as np
import pytest

import assoc_nn_shapes as ns
import cand_shapes as cs

pytestmark = pytest.mark.gpu
REPS, FILL = 2, 0x5a


@pytest.fixture(scope="module")
def S(pkg):
    """the handle with the map resident, the inputs in device memory, and check(outputs, resident, timed)"""
    if pkg.device_count() < 1:
        pytest.fail("no gfx950 device visible: the HIP path cannot run")
    b = pkg.binding; DA = b.DeviceArray
    c = ns.scene(5, 3, 8, n_poses=1, attach=1.0)
    c["map_xy"][7] = c["map_xy"][0] + [0.05, 0.0]; c["map_ty"][7] = c["map_ty"][0]            # a twin pair for the map calls
    G = pkg.Graph(lidar_to_cog=ns.LIDAR)
    G.map_append(c["map_xy"], c["map_ty"]); G.map_set_cov(0, c["map_cov"])
    n = len(c["obs"]); fs = np.array([0, n, n], dtype=np.int32); po = np.zeros(n, dtype=np.int32)
    hyp = G.assign_opt(c["poses"], po, c["obs"], fs, c["map_xy"], c["map_ty"], c["map_cov"], c["pose_cov"])[0]
    assert (hyp >= 0).any()
    two = np.concatenate([c["poses"], c["poses"] + [0.3, -0.2, 0.01]])                          # 2 hypotheses / the poses of 2 steps
    held = dict(poses=DA(c["poses"]), po=DA(po), obs=DA(c["obs"]), fs=DA(fs), pc=DA(c["pose_cov"]), hyp=DA(hyp), two=DA(two),
                two_cov=DA(np.concatenate([c["pose_cov"]] * 2)), motion=DA(np.array([[0.1, 0.0, 0.0]])), motion_cov=DA(c["pose_cov"] * 0.01),
                in_idx=DA(np.full(n, -1, dtype=np.int32)), table=DA(cs.far_records(2).view(np.uint8)))

    def check(outputs, resident, timed):
        """outputs: {name: bytes}; resident(bufs) and timed(bufs) make the two calls on a dict of fresh DeviceArrays"""
        got = []
        for call in (resident, timed):
            bufs = {k: DA(np.full(nb, FILL, dtype=np.uint8)) for k, nb in outputs.items()}
            ms = call(bufs); G.synchronize()
            got.append({k: bufs[k].to_host(np.uint8, nb).tobytes() for k, nb in outputs.items()})
            for a in bufs.values():
                a.free()
        assert np.isfinite(ms) and ms > 0, ms
        for k in outputs:
            assert got[0][k] == got[1][k], k
        assert any(v != bytes([FILL]) * len(v) for v in got[0].values()), "the resident call wrote nothing"

    yield dict(G=G, b=b, n=n, nf=2, d=held, check=check, c=c)
    for a in held.values():
        a.free()
    G.close()


def test_associate(S):
    G, d, n = S["G"], S["d"], S["n"]
    S["check"](dict(idx=4 * n),
               lambda o: G.associate_resident(d["poses"], 1, d["po"], d["obs"], n, 1.2, o["idx"], 1e-3),
               lambda o: G.time_associate_resident(d["poses"], 1, d["po"], d["obs"], n, 1.2, o["idx"], REPS, 1e-3))


def test_associate_nn(S):
    G, d, n = S["G"], S["d"], S["n"]; prm = S["b"].nn_params(gate_chi2=20.0)
    S["check"](dict(idx=4 * n, d2=8 * n, sec=8 * n),
               lambda o: G.associate_nn_resident(d["poses"], 1, d["po"], d["obs"], n, o["idx"], o["d2"], o["sec"], d["pc"], prm),
               lambda o: G.time_associate_nn_resident(d["poses"], 1, d["po"], d["obs"], n, o["idx"], REPS, o["d2"], o["sec"], d["pc"], prm))


def test_assign_nn(S):
    G, d, n, nf = S["G"], S["d"], S["n"], S["nf"]; prm = S["b"].nn_params(gate_chi2=20.0)
    S["check"](dict(idx=4 * n, d2=8 * n),
               lambda o: G.assign_nn_resident(d["poses"], 1, d["po"], d["obs"], n, nf, d["fs"], o["idx"], o["d2"], d["pc"], prm),
               lambda o: G.time_assign_nn_resident(d["poses"], 1, d["po"], d["obs"], n, nf, d["fs"], o["idx"], REPS, o["d2"], d["pc"], prm))


def test_assign_opt(S):
    G, d, n, nf = S["G"], S["d"], S["n"], S["nf"]; prm = S["b"].nn_params(gate_chi2=20.0)
    S["check"](dict(idx=4 * n, d2=8 * n, na=4 * n),
               lambda o: G.assign_opt_resident(d["poses"], 1, d["po"], d["obs"], n, nf, d["fs"], o["idx"], o["d2"], o["na"], d["pc"], prm),
               lambda o: G.time_assign_opt_resident(d["poses"], 1, d["po"], d["obs"], n, nf, d["fs"], o["idx"], REPS, o["d2"], o["na"], d["pc"], prm))


def test_joint_compat(S):
    G, d, n, nf = S["G"], S["d"], S["n"], S["nf"]; prm = S["b"].nn_params(); jc = S["b"].jc_params(0.99)
    S["check"](dict(idx=4 * n, j=8 * nf, nk=4 * nf, nd=4 * nf, nu=4 * nf, dl=24 * nf),
               lambda o: G.joint_compat_resident(d["poses"], 1, d["po"], d["obs"], n, nf, d["fs"], d["hyp"], o["idx"], o["j"], o["nk"], o["nd"], o["nu"], o["dl"],
                                                 d["pc"], prm, jc),
               lambda o: G.time_joint_compat_resident(d["poses"], 1, d["po"], d["obs"], n, nf, d["fs"], d["hyp"], o["idx"], REPS, o["j"], o["nk"], o["nd"], o["nu"],
                                                      o["dl"], d["pc"], prm, jc))


def test_localize(S):
    G, d, n, nf = S["G"], S["d"], S["n"], S["nf"]; prm = S["b"].nn_params(); loc = S["b"].loc_params(max_iterations=5)
    S["check"](dict(pose=24 * nf, cov=72 * nf, chi2=8 * nf, pairs=4 * nf, it=4 * nf, st=4 * nf),
               lambda o: G.localize_resident(d["poses"], 1, d["po"], d["obs"], n, nf, d["fs"], d["hyp"], o["pose"], o["cov"], o["chi2"], o["pairs"], o["it"], o["st"],
                                             d["pc"], prm, loc),
               lambda o: G.time_localize_resident(d["poses"], 1, d["po"], d["obs"], n, nf, d["fs"], d["hyp"], REPS, o["pose"], o["cov"], o["chi2"], o["pairs"], o["it"],
                                                  o["st"], d["pc"], prm, loc))


def test_relocalize(S):
    G, d, n, nf = S["G"], S["d"], S["n"], S["nf"]; prm = S["b"].reloc_params(min_inliers=2)
    S["check"](dict(pose=24 * nf, count=4 * nf, cost=8 * nf, seed=16 * nf, sc=4 * nf, sp=24 * nf, ns=8 * nf, st=4 * nf, idx=4 * n, e2=8 * n),
               lambda o: G.relocalize_resident(d["obs"], n, nf, d["fs"], o["pose"], o["count"], o["cost"], o["seed"], o["sc"], o["sp"], o["ns"], o["st"], o["idx"],
                                               o["e2"], prm),
               lambda o: G.time_relocalize_resident(d["obs"], n, nf, d["fs"], REPS, o["pose"], o["count"], o["cost"], o["seed"], o["sc"], o["sp"], o["ns"], o["st"],
                                                    o["idx"], o["e2"], prm))


def test_follow(S):
    G, b, d, n = S["G"], S["b"], S["d"], S["n"]
    blk = (b.nn_params(), b.jc_params(), b.loc_params(), b.follow_params(min_pairs=1))
    S["check"](dict(steps=2 * 2 * b.FOLLOW_STEP.itemsize, idx=4 * 2 * n, state=2 * b.FOLLOW_STATE.itemsize, best=8),
               lambda o: G.follow_resident(d["two"], 2, d["obs"], n, 2, d["fs"], n, d["motion"], d["two_cov"], d["motion_cov"], o["steps"], o["idx"], o["state"],
                                           o["best"], *blk),
               lambda o: G.time_follow_resident(d["two"], 2, d["obs"], n, 2, d["fs"], n, REPS, d["motion"], d["two_cov"], d["motion_cov"], o["steps"], o["idx"],
                                                o["state"], o["best"], *blk))


def test_cand(S):
    G, b, d, n = S["G"], S["b"], S["d"], S["n"]; blk = (b.nn_params(), b.cand_params(confirm_hits=1))
    S["check"](dict(steps=2 * b.CAND_STEP.itemsize, cid=4 * n, slot=4 * n, tab=b.CAND_MAX * b.CAND.itemsize, meta=16),
               lambda o: G.cand_resident(d["obs"], n, 2, d["fs"], n, d["two"], d["two_cov"], d["in_idx"], 2, d["table"], o["steps"], o["cid"], o["slot"], o["tab"],
                                         o["meta"], *blk),
               lambda o: G.time_cand_resident(d["obs"], n, 2, d["fs"], n, d["two"], REPS, d["two_cov"], d["in_idx"], 2, d["table"], o["steps"], o["cid"], o["slot"],
                                              o["tab"], o["meta"], *blk))


def test_map_twins_and_the_merge_that_leaves_the_map(S):
    G, b = S["G"], S["b"]; prm = b.dup_params(max_distance=0.5); m = G.map_size()
    assert m == 8
    S["check"](dict(tw=4 * m, d2=8 * m, sec=8 * m, na=4 * m),
               lambda o: G.map_twins_resident(o["tw"], o["d2"], o["sec"], o["na"], prm),
               lambda o: G.time_map_twins_resident(o["tw"], REPS, o["d2"], o["sec"], o["na"], prm))
    assert (G.map_twins(S["c"]["map_xy"], S["c"]["map_ty"], S["c"]["map_cov"], prm)[0] >= 0).sum() == 2       # the planted pair: a merge has work to do
    before = (G.map_xy(), G.map_cov())
    ms = G.time_map_merge_twins(REPS, prm)
    assert np.isfinite(ms) and ms > 0, ms
    after = (G.map_xy(), G.map_cov())
    assert G.map_size() == m and before[0][0].tobytes() == after[0][0].tobytes() and before[0][1].tobytes() == after[0][1].tobytes()
    assert before[1].tobytes() == after[1].tobytes()
