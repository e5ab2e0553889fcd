#!/usr/bin/env python3
"""Do gs_optimize_lm, gs_optimize_dogleg and gs_multiply_hessian of this tree's library compute, bit for bit, what another build of
the library computes, and in the same time?  (Needs a gfx950 GPU.)

    make -C <other tree>/csrc variant NAME=parent      # then copy or link its build/var_parent/libgraphslam_hip.so under this tree's csrc/build/var_parent/
    scripts/trial_vs_parent.py [OTHER_LIB] > profiles/<name>.txt

Each library runs in a child process of its own (the other one through GS_LIB).  Cases, for both methods: bench 1000 / 200 from x1 of
tests/test_lm_cpu.starts(seed 1), 6 iterations — LM with initial_lambda 1e-12 and the default, the dogleg with defaults and
initial_delta 1 — on the fused path, with linearize_gather = 1, with factor_variant = 4 and with tree = 0; the grown plan of
tests/test_gpu_lm.grown; the robust + prior + polar + inactive-edge case of tests/test_dogleg_cpu.side_case; the graphs with
N + M = 255, 256, 257 of tests/test_lm_cpu.boundary_start; one Hessian product per graph.  Poses, landmarks, every field of the info
dict and chi2_initial / chi2_final / iterations / numeric_failure / first_failure of the stats are compared byte by byte.

Then the time: bench 10k / 2k from the graph's own start, optimize_lm(6) and optimize_dogleg(6), stats.ms_total (the device interval of
the call) of five calls per library after a warm one, the two libraries alternating call by call, each call on a fresh handle.
Exit status 1 when anything differs (the times are reported, not judged)."""
import importlib
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = ("chi2_initial", "chi2_final", "iterations", "numeric_failure", "first_failure")
METHODS = {"lm": [dict(initial_lambda=1e-12), {}], "dogleg": [{}, dict(initial_delta=1.0)]}


def setup():
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    pkg = importlib.import_module("opendlv-logic-cfsd18-sensation-slam_amd")
    pkg.binding.DEFAULT_DEBUG["grow_min_poses"] = 0                 # as the tests' pkg fixture: plans of every size may grow
    from oracle import pyoracle as po
    fe = po.OracleFrontend(); cache = {}

    def bench_graphs(N, M):
        if (N, M) not in cache:
            t = pkg.track.generate(N, M); cache[(N, M)] = (t, pkg.track.bench_graph(t, fe))
        return cache[(N, M)]
    return pkg, po, bench_graphs


def child(path):
    pkg, po, bench_graphs = setup()
    import test_dogleg_cpu, test_gpu_dogleg, test_gpu_lm, test_lm_cpu
    out = {}

    def record(name, make):
        """both methods with both parameter sets on handles of make(); then one Hessian product on the last handle's last linearisation"""
        rng = np.random.default_rng(11)
        for method, sets in METHODS.items():
            for k, kw in enumerate(sets):
                G = make(); key = "%s/%s%d" % (name, method, k)
                done, st, info = (G.optimize_lm if method == "lm" else G.optimize_dogleg)(6, **kw)
                out[key + "/poses"] = G.poses(); out[key + "/lms"] = G.landmarks(); out[key + "/done"] = np.int64(done)
                for f in STATS:
                    out[key + "/stats." + f] = np.asarray(getattr(st, f))
                for f, v in info.items():
                    out[key + "/info." + f] = np.asarray(v)
                print("%-28s accepted %d trials %s rejected %d chi2 %.9g -> %.9g" % (key, done, info["n_trials"][:max(done, 1)].tolist(), info["rejected"], st.chi2_initial, st.chi2_final), flush=True)
                if method == "dogleg" and k == 1:
                    P, L = G.poses(), G.landmarks()
                    yp, yl = G.multiply_hessian(rng.normal(size=P.shape), rng.normal(size=L.shape))
                    out[name + "/hmul_pose"] = yp; out[name + "/hmul_lm"] = yl
                G.close()

    g, _, _, P1, L1, _, _ = test_lm_cpu.starts(po, bench_graphs, 1)
    gs = dict(g, pose_est=P1, lm_est=L1)
    for label, kw in (("x1", {}), ("x1_gather", dict(linearize_gather=1)), ("x1_variant4", dict(factor_variant=4)), ("x1_tree0", dict(debug=dict(tree=0)))):
        record(label, lambda: test_gpu_lm.fresh(pkg, gs, **kw))
    record("grown", lambda: test_gpu_lm.grown(pkg, bench_graphs(1000, 200)[1])[0])
    side = test_dogleg_cpu.side_case(po, bench_graphs)[1:]
    record("side", lambda: test_gpu_dogleg.side_handle(pkg, *side))
    for total in sorted(test_lm_cpu.BOUNDARY):
        gb, Pb, Lb = test_lm_cpu.boundary_start(po, bench_graphs, total)
        record("n%d" % total, lambda: test_gpu_lm.fresh(pkg, dict(gb, pose_est=Pb, lm_est=Lb)))
    for k, v in out.items():
        assert np.all(np.isfinite(np.asarray(v, dtype=np.float64))), k
    np.savez(path, **out)


def timer():
    """one line per request on stdin ("lm" / "dogleg"): ms_total of a 6-iteration call on a fresh handle holding bench 10k / 2k"""
    pkg, po, bench_graphs = setup()
    g = bench_graphs(10000, 2000)[1]
    print("ready", flush=True)
    for line in sys.stdin:
        G = pkg.Graph(device=0); G.load_bench_graph(g)
        done, st, info = (G.optimize_lm if line.strip() == "lm" else G.optimize_dogleg)(6)
        G.close()
        print("%.6f %d %d" % (st.ms_total, done, info["trials"]), flush=True)


def timing(libs, lines):
    procs = {}
    for label, env in libs:
        procs[label] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--timer"], env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    try:
        for label, p in procs.items():
            if p.stdout.readline().strip() != "ready":
                lines.append("timing: the %s child did not start" % label); return False
        lines.append("== time: bench 10k / 2k, 6 iterations from the graph's own start, stats.ms_total [ms], 1 warm + 5 calls, libraries alternating")
        for method in ("lm", "dogleg"):
            ms = {label: [] for label in procs}
            for rep in range(6):
                for label, p in procs.items():
                    p.stdin.write(method + "\n"); p.stdin.flush()
                    ans = p.stdout.readline().split()
                    if len(ans) != 3:
                        lines.append("timing: the %s child ended in a %s call" % (label, method)); return False      # nothing more on the GPU after a failure
                    if rep:
                        ms[label].append(float(ans[0]))
            for label, v in ms.items():
                lines.append("%-7s %-7s median %.3f  min %.3f  max %.3f   %s" % (method, label, float(np.median(v)), min(v), max(v), " ".join("%.3f" % x for x in v)))
            a, m = ms["parent"], float(np.median(ms["new"]))
            lines.append("%-7s this tree's median %s the parent's min - max" % (method, "lies within" if min(a) <= m <= max(a) else
                                                                              ("lies BELOW (faster than)" if m < min(a) else "lies ABOVE (slower than)")))
        return True
    finally:
        for p in procs.values():
            p.stdin.close(); p.wait(timeout=60)


def main():
    OUT = tempfile.mkdtemp()
    PARENT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "opendlv-logic-cfsd18-sensation-slam_amd", "csrc", "build", "var_parent", "libgraphslam_hip.so")
    lines, libs = [], []
    for label, lib in (("parent", PARENT), ("new", None)):
        env = dict(os.environ)
        if lib:
            env["GS_LIB"] = lib
        else:
            env.pop("GS_LIB", None)
        libs.append((label, env))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", os.path.join(OUT, label + ".npz")], env=env,
                           capture_output=True, text=True, timeout=400)
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
        if not same:
            lines.append("%-40s %-10s DIFFERENT (max abs diff %.3g)" % (k, "x".join(map(str, a[k].shape)), np.abs(a[k].astype(float) - b[k].astype(float)).max()))
    groups = sorted(set(k.rsplit("/", 1)[0] for k in a.files))
    lines.append("%d arrays in %d groups (%s)" % (len(a.files), len(groups), " ".join(groups)))
    lines.append("verdict: %s" % ("all %d arrays bit-identical" % len(a.files) if not bad else "%d arrays differ" % bad))
    ok = True if bad else timing(libs, lines)
    print("\n".join(lines))
    sys.exit(1 if bad or not ok else 0)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    elif len(sys.argv) == 2 and sys.argv[1] == "--timer":
        timer()
    else:
        main()
