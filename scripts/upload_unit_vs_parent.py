#!/usr/bin/env python3
"""Does this tree's library compute, bit for bit, what another build of it computes through the upload paths?  (Needs a gfx950 GPU.)

    make -C <other tree>/csrc variant NAME=parent      # then copy or link its build/var_parent/libgraphslam_hip.so under this tree's csrc/build/var_parent/
    scripts/upload_unit_vs_parent.py [OTHER_LIB] > profiles/<name>.txt

Each library runs in a child process of its own (the other one through GS_LIB): cfg1, cfg3 and a track with workgroup fronts (16 cones in
view) without their last pose through optimize(10), then that pose appended — one growth step where the plan grows — and optimize(10)
again; cfg3 as 4 pose-window handles on one GPU, 10 iterations.  Every array of estimates is compared byte by byte.  Exit status 1 when
anything differs."""
import importlib
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(path):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import split_for_growth, append_tail
    pkg = importlib.import_module("opendlv-logic-cfsd18-sensation-slam_amd")
    out = {}
    fe = pkg.Graph(device=0)


    def fresh(arrays, **kw):
        g = pkg.Graph(**kw); g.load_bench_graph(arrays); return g


    def grow_case(name, N, M, K=None):
        t = pkg.track.generate(N, M, K) if K else pkg.track.generate(N, M)
        g = pkg.track.bench_graph(t, fe)
        base, tail, full = split_for_growth(g, 1)
        G = fresh(base); done, st = G.optimize(10)
        out[name + "/poses10"] = G.poses(); out[name + "/lms10"] = G.landmarks()
        append_tail(G, tail); done2, st2 = G.optimize(10)
        out[name + "/poses20"] = G.poses(); out[name + "/lms20"] = G.landmarks()
        out[name + "/meta"] = np.array([done, done2, G.plan_growths(), st.max_front, st.factor_variant, st2.n_fronts], dtype=np.int64)
        print("%s: %d + %d iterations, growths %d (%s), max front %d, variant %d, chi2 %.9g -> %.9g" %
              (name, done, done2, G.plan_growths(), G.growth_refusal() or "grown", st.max_front, st.factor_variant, st.chi2_initial, st2.chi2_final), flush=True)
        G.close()
        return g


    grow_case("cfg1", 50, 30)
    g3 = grow_case("cfg3", 10000, 2000)
    grow_case("wg_K16", 1000, 200, 16)
    # 4 pose-window handles on one GPU, exchange buffers summed in-process (tests/test_gpu_parity.py: test_sharded_iterations_match_oracle)
    world = 4; ranks = []
    for r in range(world):
        G = fresh(g3, debug=dict(shard_by_window=1)); G.dist_configure(r, world); G.initialize_optimization(); ranks.append(G)
    for _ in range(10):
        for G in ranks:
            G.dist_iterate_local()
        total = sum(G.dist_read_exchange() for G in ranks)
        for G in ranks:
            G.dist_write_exchange(total); G.dist_iterate_finish()
    for r, G in enumerate(ranks):
        G.sync_estimates()
        out["shard4/poses_r%d" % r] = G.poses(); out["shard4/lms_r%d" % r] = G.landmarks(); out["shard4/exchange_r%d" % r] = G.dist_read_exchange()
        G.close()
    print("shard4: 10 iterations on 4 handles, exchange %d doubles" % len(total), flush=True)
    fe.close()
    for k, v in out.items():
        assert np.all(np.isfinite(np.asarray(v, dtype=np.float64))), k
    np.savez(path, **out)


def main():
    OUT = tempfile.mkdtemp(); os.makedirs(OUT, exist_ok=True)
    PARENT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "opendlv-logic-cfsd18-sensation-slam_amd", "csrc", "build", "var_parent", "libgraphslam_hip.so")
    lines = []
    for label, lib in (("parent", PARENT), ("new", None)):
        env = dict(os.environ)
        if lib:
            env["GS_LIB"] = lib
        else:
            env.pop("GS_LIB", None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", os.path.join(OUT, label + ".npz")], env=env,
                           capture_output=True, text=True, timeout=240)
        lines.append("== %s (%s), exit %d\n%s%s" % (label, os.path.relpath(lib, ROOT) if lib else "the tree's library", r.returncode, r.stdout, r.stderr[-2000:]))
        if r.returncode != 0:
            print("\n".join(lines)); sys.exit(1)   # nothing more on the GPU after a failure
    a = np.load(os.path.join(OUT, "parent.npz")); b = np.load(os.path.join(OUT, "new.npz"))
    bad = 0
    lines.append("== comparison (bitwise: same dtype, shape and bytes)")
    assert sorted(a.files) == sorted(b.files)
    for k in sorted(a.files):
        same = a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()
        bad += not same
        lines.append("%-22s %-14s %s" % (k, "x".join(map(str, a[k].shape)), "identical" if same else "DIFFERENT (max abs diff %.3g)" % np.abs(a[k].astype(float) - b[k].astype(float)).max()))
    lines.append("verdict: %s" % ("all %d arrays bit-identical" % len(a.files) if not bad else "%d arrays differ" % bad))
    print("\n".join(lines))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
