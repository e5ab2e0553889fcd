"""Checker of edge deactivation (numpy only).

An inactive edge is an edge whose information matrix is zero: `masked(g, act_pp, act_pl)` is the graph dict with every edge's
information multiplied by its 0 / 1 flag, and the UNCHANGED CPU oracle on that graph is the reference for H, b, chi2, iterations and
LM — a zero-information edge adds exact zeros there too.  test_edge_mask_cpu.py pins this against the oracle on the graph with those
edges physically left out (`without`).

Also here, restated in plain Python from include/graphslam.h: the scan for isolated vertices (a FREE vertex that carries no prior and
has no active edge; poses in insertion order, then landmarks) and the keep_connected rule of gs_deactivate_edges_above (candidates in
insertion order; one is skipped when it would leave a free, prior-less endpoint without an active edge, given the decisions so far)."""
import numpy as np


def masked(g, act_pp, act_pl):
    """copy of the graph dict with pp_info / pl_info rows multiplied by the edge's flag (1 active, 0 inactive)"""
    out = dict(g)
    out["pp_info"] = np.asarray(g["pp_info"], dtype=np.float64).reshape(-1, 9) * np.asarray(act_pp, dtype=np.float64)[:, None]
    out["pl_info"] = np.asarray(g["pl_info"], dtype=np.float64).reshape(-1, 4) * np.asarray(act_pl, dtype=np.float64)[:, None]
    return out


def without(g, act_pp, act_pl):
    """the graph with the inactive edges physically left out; edge k of the result is edge flatnonzero(act)[k] of g"""
    a, b = np.asarray(act_pp, dtype=bool), np.asarray(act_pl, dtype=bool)
    out = dict(g)
    for k in ("pp_i", "pp_j", "pp_z", "pp_info"):
        out[k] = np.asarray(g[k])[a]
    for k in ("pl_p", "pl_l", "pl_z", "pl_info"):
        out[k] = np.asarray(g[k])[b]
    return out


def _free_without_prior(g, pose_prior=(), lm_prior=()):
    need_p = np.ones(len(g["pose_est"]), dtype=bool); need_l = np.ones(len(g["lm_est"]), dtype=bool)
    need_p[np.asarray(g["fixed_poses"], dtype=np.int64)] = False; need_l[np.asarray(g["fixed_landmarks"], dtype=np.int64)] = False
    need_p[np.asarray(list(pose_prior), dtype=np.int64)] = False; need_l[np.asarray(list(lm_prior), dtype=np.int64)] = False
    return need_p, need_l


def degrees(g, act_pp, act_pl):
    """active edges per pose / per landmark"""
    dp = np.zeros(len(g["pose_est"]), dtype=np.int64); dl = np.zeros(len(g["lm_est"]), dtype=np.int64)
    a, b = np.asarray(act_pp, dtype=bool), np.asarray(act_pl, dtype=bool)
    np.add.at(dp, np.asarray(g["pp_i"])[a], 1); np.add.at(dp, np.asarray(g["pp_j"])[a], 1)
    np.add.at(dp, np.asarray(g["pl_p"])[b], 1); np.add.at(dl, np.asarray(g["pl_l"])[b], 1)
    return dp, dl


def isolated_vertex(g, act_pp, act_pl, pose_prior=(), lm_prior=()):
    """("pose" | "landmark", index) of the first isolated vertex, or None"""
    need_p, need_l = _free_without_prior(g, pose_prior, lm_prior)
    dp, dl = degrees(g, act_pp, act_pl)
    for p in range(len(dp)):
        if need_p[p] and dp[p] == 0:
            return "pose", p
    for l in range(len(dl)):
        if need_l[l] and dl[l] == 0:
            return "landmark", l
    return None


def deactivate(g, act_pp, act_pl, kind, cand, keep_connected, pose_prior=(), lm_prior=()):
    """gs_deactivate_edges_above's host half: (new act_pp, new act_pl, indices newly switched off)"""
    act = [np.array(act_pp, dtype=bool, copy=True), np.array(act_pl, dtype=bool, copy=True)]
    kd = {"odometry": 0, "observation": 1}.get(kind, kind)
    need_p, need_l = _free_without_prior(g, pose_prior, lm_prior)
    dp, dl = degrees(g, act[0], act[1])
    off = []
    for k in np.flatnonzero(np.asarray(cand, dtype=bool)):
        if not act[kd][k]:
            continue
        if kd == 0:
            ends = [(need_p, dp, int(g["pp_i"][k])), (need_p, dp, int(g["pp_j"][k]))]
        else:
            ends = [(need_p, dp, int(g["pl_p"][k])), (need_l, dl, int(g["pl_l"][k]))]
        lim = 2 if kd == 0 and ends[0][2] == ends[1][2] else 1          # (a self-edge counts twice in its vertex's degree)
        if keep_connected and any(need[v] and deg[v] <= lim for need, deg, v in ends):
            continue
        for _, deg, v in ends:
            deg[v] -= 1
        act[kd][k] = False; off.append(int(k))
    return act[0], act[1], np.array(off, dtype=np.int64)


def random_masks(g, seed, share=0.1):
    """(act_pp, act_pl): about `share` of each kind switched off by a seeded RNG, in an order-independent way that isolates no vertex
    (an edge whose removal would isolate an endpoint, given the edges already taken, stays)"""
    rng = np.random.default_rng(seed)
    act = [np.ones(len(g["pp_i"]), dtype=bool), np.ones(len(g["pl_p"]), dtype=bool)]
    for kd in (0, 1):
        n = len(act[kd]); cand = np.zeros(n, dtype=bool); cand[rng.choice(n, max(1, int(round(share * n))), replace=False)] = True
        act[0], act[1], _ = deactivate(g, act[0], act[1], kd, cand, True)
    assert isolated_vertex(g, act[0], act[1]) is None
    return act[0], act[1]


def widest_gap_threshold(s, floor):
    """(threshold, relative gap): the midpoint of the widest relative gap (hi - lo) / hi between consecutive sorted values, looked for
    from the gate region up: the values above `floor` and the largest value at or below it.  floor = the square of the robust kernel's
    delta: below it the kernel treats an edge as an inlier (weight 1), so no gate belongs there — and among the near-zero values of
    well-fitted edges (1e-34 next to 1e-9) the widest RATIO of the whole array is found, which separates nothing."""
    v = np.sort(np.asarray(s, dtype=np.float64))
    first = max(int(np.searchsorted(v, floor, side="right")) - 1, 0)
    v = v[first:]
    r = (v[1:] - v[:-1]) / v[1:]
    k = int(np.argmax(r))
    return 0.5 * (v[k] + v[k + 1]), float(r[k])
