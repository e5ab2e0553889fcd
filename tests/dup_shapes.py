"""Scenes of the map twins tests (TEST-ONLY): maps with planted duplicate cones, the smallest at which the kernels of gs_dup.hip can go wrong —
the tile edge of the search (256 cones), the block edge of the scan (a thread takes four blocks: 1024 cones), pairs across those edges, ties,
NaN cones, degenerate and anisotropic covariances, every parameter's other value —, the 65 536 cones the calls must work to, and the truth
scene.

A scene is a dict: name, xy [n,2], ty [n] int32, cov [n,4] or None (no covariance array at all), params (the fields of gs_dup_params that
differ from the defaults).  Base cones stand on a jittered grid of 2.5 m, at least 1.9 m apart, so only planted cones can be twins."""
import functools

import numpy as np

import relocalize_shapes as rs

DEFAULTS = dict(require_same_type=1, exclusive=0, gate_chi2=5.991464547107979, max_distance=1.0, sigma_floor=0.05)
SIZES = (0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 65536)                     # 65 536: what the calls must work to; 256 of the scan's blocks


def params_of(sc):
    p = dict(DEFAULTS); p.update(sc["params"])
    return p


def _grid(n, rng, origin=(0.0, 0.0)):
    side = max(int(np.ceil(np.sqrt(max(n, 1)))), 1)
    k = np.arange(n)
    xy = np.stack([k % side, k // side], axis=1) * 2.5 + rng.uniform(-0.3, 0.3, (n, 2)) + np.asarray(origin)
    return xy, rng.integers(0, 4, n).astype(np.int32)


def _cov_iso(n, v):
    c = np.zeros((n, 4)); c[:, 0] = c[:, 3] = v
    return c


def _cov_random(n, rng, lo=0.002, hi=0.02):
    """symmetric positive definite blocks with eigenvalues in [lo, hi] and any orientation, bitwise symmetric"""
    a = rng.uniform(0, np.pi, n); e0 = rng.uniform(lo, hi, n); e1 = rng.uniform(lo, hi, n); c, s = np.cos(a), np.sin(a)
    c00 = e0 * c * c + e1 * s * s; c01 = (e0 - e1) * c * s; c11 = e0 * s * s + e1 * c * c
    return np.stack([c00, c01, c01, c11], axis=1)


def _pack(name, xy, ty, cov, **params):
    xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2); ty = np.ascontiguousarray(ty, dtype=np.int32).reshape(-1)
    cov = None if cov is None else np.ascontiguousarray(cov, dtype=np.float64).reshape(-1, 4)
    assert len(ty) == len(xy) and (cov is None or len(cov) == len(xy))
    return dict(name=name, xy=xy, ty=ty, cov=cov, params=params)


def _planted(name, n, seed, cov="random", sigma=0.06, shuffle=True, **params):
    """n cones in all: n // 8 of them (n // 100 of a large map) copies of a base cone displaced by N(0, sigma), everything in a random order"""
    rng = np.random.default_rng(seed)
    n_tw = n // 100 if n > 4096 else n // 8 if n > 2 else n // 2
    nb = n - n_tw
    xy, ty = _grid(nb, rng)
    cv = None if cov is None else _cov_random(nb, rng) if cov == "random" else _cov_iso(nb, cov)
    src = rng.choice(nb, n_tw, replace=False) if n_tw else np.zeros(0, dtype=np.int64)
    xy = np.concatenate([xy, xy[src] + rng.normal(0, sigma, (n_tw, 2))]); ty = np.concatenate([ty, ty[src]])
    if cv is not None:
        cv = np.concatenate([cv, _cov_random(n_tw, rng) if cov == "random" else _cov_iso(n_tw, cov)])
    if shuffle and n > 1:
        o = rng.permutation(n); xy, ty = xy[o], ty[o]; cv = None if cv is None else cv[o]
    return _pack(name, xy, ty, cv, **params)


def _placed(name, n, seed, places, cov_v=0.0072, **params):
    """a base map of n cones with the listed (index, xy, type) written over it (far from the grid: x around -50)"""
    rng = np.random.default_rng(seed)
    xy, ty = _grid(n, rng); cv = _cov_iso(n, cov_v)
    for item in places:
        i, p, t = item[:3]
        xy[i] = p; ty[i] = t
        if len(item) > 3:
            cv[i] = item[3]
    return _pack(name, xy, ty, cv, **params)


def truth():
    """relocalize_shapes.track()'s 120 cones with every third one mapped a second time at the end, displaced by N(0, 0.12); every covariance
    (0.12^2 / 2) I; default parameters.  Returns (scene, planted pairs [(a, b)])"""
    xy, ty, _ = rs.track()
    src = np.arange(0, 120, 3)
    d = np.random.default_rng(31).normal(0, 0.12, (40, 2))
    xy2 = np.concatenate([xy, xy[src] + d]); ty2 = np.concatenate([ty, ty[src]])
    sc = _pack("truth", xy2, ty2, _cov_iso(160, 0.12 * 0.12 / 2))
    return sc, [(int(a), 120 + k) for k, a in enumerate(src)]


def _special(name):
    F = -50.0                                                                  # where the hand-placed cones stand
    if name == "straddle":                                                     # a twin pair across the tile edge
        return _placed(name, 300, 1, [(255, (F, 0.0), 1), (256, (F + 0.1, 0.05), 1)])
    if name == "ends":                                                         # a pair at (0, n - 1)
        return _placed(name, 600, 2, [(0, (F, 0.0), 2), (599, (F - 0.08, 0.06), 2)])
    if name == "triplet":                                                      # 0.0, 0.1, 0.25 on a line: two rounds
        return _placed(name, 40, 3, [(7, (F, 0.0), 1), (21, (F + 0.1, 0.0), 1), (30, (F + 0.25, 0.0), 1)])
    if name in ("tie", "tie_exclusive"):                                       # mirrored around (F, 8): the centre's two d2 are equal bits
        pl = [(3, (F, 8.0), 1), (5, (F - 0.25, 8.0), 1), (9, (F + 0.25, 8.0), 1)]
        return _placed(name, 20, 4, pl, **({"exclusive": 1} if name == "tie_exclusive" else {}))
    if name in ("type_mismatch", "type_ignored"):                              # two cones of different type at one place
        pl = [(2, (F, 3.0), 1), (11, (F, 3.0), 2)]
        return _placed(name, 16, 5, pl, **({"require_same_type": 0} if name == "type_ignored" else {}))
    if name == "gate_not_distance":                                            # wide covariances 1.2 m apart: inside the gate, outside max_distance
        w = (0.5, 0.0, 0.0, 0.5)
        return _placed(name, 16, 6, [(1, (F, 0.0), 1, w), (8, (F + 1.2, 0.0), 1, w)])
    if name == "distance_not_gate":                                            # tight covariances 0.3 m apart: inside max_distance, outside the gate
        t = (1e-4, 0.0, 0.0, 1e-4)
        return _placed(name, 16, 7, [(1, (F, 0.0), 1, t), (8, (F + 0.3, 0.0), 1, t)])
    if name == "nan_between":                                                  # a NaN cone between two twins
        return _placed(name, 12, 8, [(4, (F, 0.0), 1), (5, (np.nan, np.nan), 1), (6, (F + 0.07, -0.04), 1)])
    if name == "zero_cov":
        return _planted(name, 130, 9, cov=0.0)
    if name == "zero_floor_zero_cov":                                          # det = 0 everywhere: nothing admissible
        return _planted(name, 130, 9, cov=0.0, sigma_floor=0.0)
    if name == "anisotropic":
        rng = np.random.default_rng(10); sc = _planted(name, 200, 10)
        sc["cov"] = np.ascontiguousarray(_cov_random(200, rng, lo=0.0004, hi=0.04))
        return sc
    if name == "no_cov":
        return _planted(name, 300, 11, cov=None)
    if name == "all_paired":                                                   # 256 cones and a twin of each, twins behind their originals
        rng = np.random.default_rng(12); xy, ty = _grid(256, rng)
        return _pack(name, np.concatenate([xy, xy + rng.normal(0, 0.05, (256, 2))]), np.concatenate([ty, ty]), _cov_iso(512, 0.0072))
    if name == "truth":
        return truth()[0]
    raise KeyError(name)


SPECIAL = ("straddle", "ends", "triplet", "tie", "tie_exclusive", "type_mismatch", "type_ignored", "gate_not_distance", "distance_not_gate",
           "nan_between", "zero_cov", "zero_floor_zero_cov", "anisotropic", "no_cov", "all_paired", "truth")
NAMES = tuple("n%d" % n for n in SIZES) + SPECIAL


@functools.lru_cache(maxsize=None)
def scene(name):
    if name.startswith("n") and name[1:].isdigit():
        sc = _planted(name, int(name[1:]), 100 + int(name[1:]))
    else:
        sc = _special(name)
    for a in (sc["xy"], sc["ty"], sc["cov"]):
        if a is not None:
            a.setflags(write=False)
    return sc
