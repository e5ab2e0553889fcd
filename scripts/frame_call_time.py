"""Host-side latency of every live frame call (gs_frame_frontend*), one by one: the wall time of a call from Python, which is the staging, the
launches, the copies, the one wait and the copy-out.  Frames of 16 and of 256 observations along the generator's track (256: sixteen
neighbouring frames seen from one pose) against a map of 512 cones (the tile kernels) and of 4096 cones (the hashed grid), every cone with a
covariance.  Each figure is the median of `calls` calls (default 2000) after `warm` calls (default 200), in microseconds — a tenth of both
for gs_frame_frontend_relocalize, whose call is 10 to 170 ms of search on these scenes (its rows say so).

    scripts/frame_call_time.py [calls [warm]]                   one run of the library in use (GS_LIB picks another build): one JSON line
    ... --only TEXT                                             only the rows whose name holds TEXT;  --reloc-full: all `calls` for relocalisation too
    scripts/frame_call_time.py --compare LIB_A LIB_B [runs]     A and B alternately, `runs` (default 3) fresh processes each, in one session:
                                                                the table, and per row whether B's median run exceeds A's slowest run
                                                                (A's own run-to-run spread is the margin: the quantity is tens of
                                                                microseconds of host time); exit status 1 if any row does"""
import json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("frame_frontend", "frame_frontend_nn", "frame_frontend_assign", "frame_frontend_assign_opt", "frame_frontend_jc", "frame_frontend_localize",
         "frame_frontend_relocalize", "frame_frontend_follow")


def measure(calls, warm, only=None, reloc_full=False):
    import importlib
    sys.path.insert(0, ROOT)
    import numpy as np
    pkg = importlib.import_module("opendlv-logic-cfsd18-sensation-slam_amd")
    b = pkg.binding; prm, jc, loc, rl, fp = b.nn_params(), b.jc_params(), b.loc_params(), b.reloc_params(), b.follow_params()   # built once: gs_jc_params_default alone is milliseconds
    rows = {}
    for n_map in (512, 4096):
        t = pkg.track.generate(400, n_map, 16)
        G = pkg.Graph(); G.map_append(t["cone_xy"], t["cone_type"]); G.map_set_cov(0, np.tile([0.04, 0.0, 0.0, 0.04], (n_map, 1)))
        pose = t["truth_poses"][10]; cov = np.diag([0.1 ** 2, 0.1 ** 2, 0.02 ** 2]).reshape(9)
        motion, qu = np.zeros(3), np.diag([0.05 ** 2, 0.05 ** 2, 0.01 ** 2]).reshape(9)
        for k in (16, 256):
            obs = np.ascontiguousarray(t["obs"][10:10 + k // 16].reshape(-1, 4))
            todo = {"frame_frontend": lambda: G.frame_frontend(pose, obs, 2.0), "frame_frontend_nn": lambda: G.frame_frontend_nn(pose, obs, cov, prm),
                    "frame_frontend_assign": lambda: G.frame_frontend_assign(pose, obs, cov, prm), "frame_frontend_assign_opt": lambda: G.frame_frontend_assign_opt(pose, obs, cov, prm),
                    "frame_frontend_jc": lambda: G.frame_frontend_jc(pose, obs, cov, prm, jc), "frame_frontend_localize": lambda: G.frame_frontend_localize(pose, obs, cov, prm, jc, loc),
                    "frame_frontend_relocalize": lambda: G.frame_frontend_relocalize(obs, 1.0, 0.2, rl, prm, jc, loc),
                    "frame_frontend_follow": lambda: G.frame_frontend_follow(obs, motion, qu, prm, jc, loc, fp)}
            for name in CALLS:
                f = todo[name]
                if only and only not in "%s k=%d map=%d" % (name, k, n_map):
                    continue
                if name == "frame_frontend_follow":                # two hypotheses at the true pose; the run's first frame takes no motion
                    G.follow_set(np.stack([pose, pose]), np.stack([cov, cov])); G.frame_frontend_follow(obs, None, None, prm, jc, loc, fp)
                tenth = name == "frame_frontend_relocalize" and not reloc_full
                for _ in range(warm // 10 if tenth else warm):
                    f()
                dt = []
                for _ in range(calls // 10 if tenth else calls):
                    t0 = time.perf_counter(); f(); dt.append(time.perf_counter() - t0)
                row = "%s k=%d map=%d%s" % (name, k, n_map, " (%d calls)" % len(dt) if tenth else "")
                rows[row] = statistics.median(dt) * 1e6
                print("%s: %.1f us" % (row, rows[row]), file=sys.stderr, flush=True)
        G.close()
    return dict(lib=os.environ.get("GS_LIB", "(the tree's)"), calls=calls, warm=warm, median_us=rows)


def compare(lib_a, lib_b, runs, extra):
    got = {"A": [], "B": []}
    for _ in range(runs):
        for tag, lib in (("A", lib_a), ("B", lib_b)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, env=dict(os.environ, GS_LIB=os.path.abspath(lib)), stdout=subprocess.PIPE, text=True, check=True)
            got[tag].append(json.loads(out.stdout.strip().splitlines()[-1])["median_us"])
            print("run of %s done" % tag, file=sys.stderr, flush=True)
    print("live frame calls, median wall time of 2000 calls after 200 warm-up calls (relocalisation: 200 after 20), microseconds;")
    print("A = the parent's library, B = this tree's; %d fresh processes each, alternately, one session on one MI355X" % runs)
    print("%-58s %-26s %-26s %8s %8s  %s" % ("call", "A runs", "B runs", "A max", "B median", "verdict"))
    worse = 0
    for row in got["A"][0]:
        a = [r[row] for r in got["A"]]; b = [r[row] for r in got["B"]]
        bad = statistics.median(b) > max(a); worse += bad
        print("%-58s %-26s %-26s %8.1f %8.1f  %s" % (row, " ".join("%7.1f" % x for x in a), " ".join("%7.1f" % x for x in b), max(a), statistics.median(b),
                                                      "SLOWER" if bad else "ok"))
    print("verdict: %s" % ("no row of B exceeds A's slowest run" if not worse else "%d rows of B exceed A's slowest run" % worse))
    return 1 if worse else 0


if __name__ == "__main__":
    argv = sys.argv[1:]; extra = []
    if "--reloc-full" in argv:
        argv.remove("--reloc-full"); extra += ["--reloc-full"]
    only = None
    if "--only" in argv:
        i = argv.index("--only"); only = argv[i + 1]; del argv[i:i + 2]; extra += ["--only", only]
    if argv and argv[0] == "--compare":
        sys.exit(compare(argv[1], argv[2], int(argv[3]) if len(argv) > 3 else 3, extra))
    print(json.dumps(measure(int(argv[0]) if argv else 2000, int(argv[1]) if len(argv) > 1 else 200, only, "--reloc-full" in extra)))
