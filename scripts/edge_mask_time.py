"""Cost of edge deactivation: gs_time_iterations on the SAME handle with no inactive edge and with a seeded 10 % of the
observation edges inactive, interleaved rounds; the wall time of the call that applies the flags (the upload and k_edge_mask_apply behind
a gs_chi2, minus a gs_chi2 with nothing to apply) and of gs_deactivate_edges_above (upload of the tables, k_edge_select, the candidate
bytes back).  Lap size, cfg3 and cfg4.  Usage: python scripts/edge_mask_time.py [out.txt] (default profiles/edge_mask_iteration_ab.txt)."""
import importlib, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("opendlv-logic-cfsd18-sensation-slam_amd")
out = open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "edge_mask_iteration_ab.txt"), "w")


def say(line):
    print(line, flush=True); out.write(line + "\n"); out.flush()


def wall(fn):
    t0 = time.perf_counter(); r = fn(); return (time.perf_counter() - t0) * 1e3, r


say("# gs_time_iterations(20) per iteration [ms], median of 5 interleaved rounds: no inactive edge | 10 % of the observation edges inactive")
for name, (N, M) in (("lap", (1000, 200)), ("cfg3", pkg.track.CONFIGS["cfg3"]), ("cfg4", pkg.track.CONFIGS["cfg4"])):
    t = pkg.track.generate(N, M)
    fe = pkg.Graph(device=0); g = pkg.track.bench_graph(t, fe); fe.close()
    G = pkg.Graph(device=0); G.load_bench_graph(g); G.initialize_optimization()
    E = G.n_pl; rng = np.random.default_rng(21)
    deg = np.bincount(np.asarray(g["pl_l"]), minlength=M); pick = []
    for k in rng.permutation(E)[: E // 10]:                       # no cone loses its last edge
        l = int(g["pl_l"][k])
        if deg[l] > 1:
            deg[l] -= 1; pick.append(int(k))
    pick = np.sort(np.array(pick, dtype=np.int32))
    rounds = {"without": [], "with": []}; apply_ms = []; restore_ms = []
    G.chi2()
    for r in range(5):
        G.activate_all_edges(); ms_r, _ = wall(G.chi2); base_ms, _ = wall(G.chi2)
        s = G.time_iterations(20); rounds["without"].append((s.ms_total, s.ms_linearize))
        G.set_edges_active("observation", pick); ms_a, _ = wall(G.chi2); base2, _ = wall(G.chi2)
        s = G.time_iterations(20); rounds["with"].append((s.ms_total, s.ms_linearize))
        apply_ms.append(ms_a - base2); restore_ms.append(ms_r - base_ms)
    assert G.find_isolated_vertex() is None
    med = {k: np.median(np.array(v), axis=0) for k, v in rounds.items()}
    G.activate_all_edges(); G.chi2()
    s_all, _ = G.edge_chi2("observation"); thr = float(np.quantile(s_all, 0.99))
    sel = []
    for r in range(5):
        G.activate_all_edges(); G.chi2()
        ms, n_off = wall(lambda: G.deactivate_edges_above("observation", thr, keep_connected=True)); sel.append(ms)
    say("%-5s %7d poses %6d cones %8d observation edges, %7d inactive: iteration %.4f | %.4f ms (x%.4f), linearise phase %.4f | %.4f ms"
        % (name, N, M, E, len(pick), med["without"][0], med["with"][0], med["with"][0] / med["without"][0], med["without"][1], med["with"][1]))
    say("      applying %d flags (upload + k_edge_mask_apply + wait, wall, median of 5): %.3f ms; restoring them: %.3f ms; gs_deactivate_edges_above over %d edges (tables up, k_edge_select, bytes back, host walk; %d switched off): %.3f ms"
        % (len(pick), float(np.median(apply_ms)), float(np.median(restore_ms[1:])), E, n_off, float(np.median(sel))))
    G.close()
