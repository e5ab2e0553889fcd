"""Map twins next to what the library offered before them, in ONE session on one handle: maps of 240, 10 000 (the benchmark's map) and 65 536
cones on a jittered grid of 2.5 m, 1 % of them mapped a second time 0.1 m (sigma) beside themselves, covariance (0.12^2 / 2) I.

    twins_ms     gs_debug_time_map_twins_resident: HIP events on the search's dispatch, mean of `reps` calls
    merge_ms     gs_debug_time_map_merge_twins: HIP events from the search to the scatter (the four dispatches of gs_map_merge_twins; the map is
                 left as it is, so every run sees the same twins), mean of `reps` runs
    merge_call_ms  one gs_map_merge_twins call, wall clock, with its copies back and its wait (then the map is set again)
    host_ms      what a caller of the parent commit has to do instead: the rule in numpy on its own host copy of the map (candidate pairs from
                 a KD-tree where scipy is installed, brute force in blocks otherwise), then gs_map_clear + gs_map_append + gs_map_set_cov of
                 the consolidated map, wall clock, best of 3
Two alternating passes; the second shows how far one run moves.  One JSON line.
`--resident-only`: just the device runs (for a rocprofv3 --kernel-trace run of them alone)."""
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
pkg = importlib.import_module("opendlv-logic-cfsd18-sensation-slam_amd")
b = pkg.binding
args = [a for a in sys.argv[1:] if not a.startswith("--")]; resident_only = "--resident-only" in sys.argv
reps = int(args[0]) if len(args) > 0 else 20
SIZES = [int(a) for a in args[1:]] or [240, 10000, 65536]
try:
    from scipy.spatial import cKDTree
except ImportError:
    cKDTree = None
prm = b.dup_params()
G = pkg.Graph()
DA = b.DeviceArray


def make_map(n, seed=31):
    rng = np.random.default_rng(seed); n_tw = max(n // 100, 1); nb = n - n_tw; side = int(np.ceil(np.sqrt(nb))); k = np.arange(nb)
    xy = np.stack([k % side, k // side], axis=1) * 2.5 + rng.uniform(-0.3, 0.3, (nb, 2)); ty = rng.integers(1, 3, nb).astype(np.int32)
    src = rng.choice(nb, n_tw, replace=False)
    xy = np.concatenate([xy, xy[src] + rng.normal(0, 0.1, (n_tw, 2))]); ty = np.concatenate([ty, ty[src]])
    o = rng.permutation(n)
    cov = np.zeros((n, 4)); cov[:, 0] = cov[:, 3] = 0.12 * 0.12 / 2
    return np.ascontiguousarray(xy[o]), np.ascontiguousarray(ty[o]), cov


def host_rule(xy, ty, cov):
    """the rule in numpy: (consolidated xy, type, cov, n_pairs)"""
    n = len(xy); md = prm.max_distance; s2 = prm.sigma_floor ** 2
    if cKDTree is not None:
        pr = cKDTree(xy).query_pairs(md, output_type="ndarray")
    else:
        parts = []
        for a0 in range(0, n, 1024):
            d = np.hypot(xy[a0:a0 + 1024, None, 0] - xy[None, :, 0], xy[a0:a0 + 1024, None, 1] - xy[None, :, 1])
            i, j = np.nonzero(d < md); i += a0; parts.append(np.stack([i[i < j], j[i < j]], axis=1))
        pr = np.concatenate(parts)
    a, c = np.minimum(pr[:, 0], pr[:, 1]), np.maximum(pr[:, 0], pr[:, 1])
    ok = ty[a] == ty[c]; a, c = a[ok], c[ok]
    A = cov[a][:, [0, 1, 3]] + [s2, 0, s2]; B = cov[c][:, [0, 1, 3]] + [s2, 0, s2]; S = A + B; nu = xy[c] - xy[a]
    det = S[:, 0] * S[:, 2] - S[:, 1] ** 2
    d2 = (S[:, 2] * nu[:, 0] ** 2 - 2 * S[:, 1] * nu[:, 0] * nu[:, 1] + S[:, 0] * nu[:, 1] ** 2) / det
    ok = (np.hypot(nu[:, 0], nu[:, 1]) < md) & (det > 0) & (S[:, 0] > 0) & (d2 < prm.gate_chi2)
    a, c, d2, A, B, S, nu, det = a[ok], c[ok], d2[ok], A[ok], B[ok], S[ok], nu[ok], det[ok]
    best = np.full(n, np.inf); twin = np.full(n, -1)
    for u, v in ((a, c), (c, a)):                                             # per cone the nearest admissible partner (ties: lowest index)
        o = np.lexsort((v, d2, u)); first = np.ones(len(o), dtype=bool); first[1:] = u[o][1:] != u[o][:-1]
        uu, vv, dd = u[o][first], v[o][first], d2[o][first]
        better = (dd < best[uu]) | ((dd == best[uu]) & (vv < twin[uu])); best[uu[better]] = dd[better]; twin[uu[better]] = vv[better]
    mutual = (twin[a] == c) & (twin[c] == a)
    a, c, A, B, S, nu, det = a[mutual], c[mutual], A[mutual], B[mutual], S[mutual], nu[mutual], det[mutual]
    k00 = (A[:, 0] * S[:, 2] - A[:, 1] * S[:, 1]) / det; k01 = (A[:, 1] * S[:, 0] - A[:, 0] * S[:, 1]) / det
    k10 = (A[:, 1] * S[:, 2] - A[:, 2] * S[:, 1]) / det; k11 = (A[:, 2] * S[:, 0] - A[:, 1] * S[:, 1]) / det
    oxy = xy.copy(); ocv = cov.copy()
    oxy[a] = xy[a] + np.stack([k00 * nu[:, 0] + k01 * nu[:, 1], k10 * nu[:, 0] + k11 * nu[:, 1]], axis=1)
    f01 = k00 * B[:, 1] + k01 * B[:, 2]
    ocv[a] = np.stack([k00 * B[:, 0] + k01 * B[:, 1], f01, f01, k10 * B[:, 1] + k11 * B[:, 2]], axis=1)
    keep = np.ones(n, dtype=bool); keep[c] = False
    return oxy[keep], ty[keep], ocv[keep], len(a)


def set_map(xy, ty, cov):
    G.map_clear(); G.map_append(xy, ty); G.map_set_cov(0, cov)


out = dict(reps=reps, kdtree=cKDTree is not None, runs={})
for rnd in range(2):
    for n in SIZES:
        xy, ty, cov = make_map(n)
        set_map(xy, ty, cov); G.synchronize()
        d_tw, d_d2, d_sec, d_na = DA(np.zeros(n, dtype=np.int32)), DA(np.zeros(n)), DA(np.zeros(n)), DA(np.zeros(n, dtype=np.int32))
        r = out["runs"].setdefault(str(n), {})
        r["twins_ms_%d" % rnd] = G.time_map_twins_resident(d_tw, reps, d_d2, d_sec, d_na, prm)
        r["merge_ms_%d" % rnd] = G.time_map_merge_twins(reps, prm)
        t0 = time.perf_counter(); _, info = G.map_merge_twins(prm); r["merge_call_ms_%d" % rnd] = (time.perf_counter() - t0) * 1e3
        r["n_pairs"] = int(info["n_pairs"]); r["n_out"] = int(info["n_out"])
        dev_xy = G.map_xy()[0]
        if not resident_only:
            best = float("inf")
            for _ in range(3):
                t0 = time.perf_counter()
                oxy, oty, ocv, npairs = host_rule(xy, ty, cov)
                set_map(oxy, oty, ocv); G.synchronize()
                best = min(best, (time.perf_counter() - t0) * 1e3)
            r["host_ms_%d" % rnd] = best; r["host_n_pairs"] = npairs
            r["host_vs_device_max_abs_xy"] = float(np.abs(oxy - dev_xy).max()) if len(oxy) == len(dev_xy) else None
            r["ratio_host_over_merge_call_%d" % rnd] = best / r["merge_call_ms_%d" % rnd]
        for a in (d_tw, d_d2, d_sec, d_na):
            a.free()
out["note"] = "a consolidation is four dispatches: k_dup_nearest, k_dup_fuse, k_dup_scan, k_dup_scatter; a query is k_dup_nearest alone"
print(json.dumps(out))
G.close()
