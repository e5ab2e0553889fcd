"""A Python execution of the device front end (TEST-ONLY), step for step as the kernels' comments describe it — what plan_exec.py and
selinv_exec.py are for their algorithms: the numpy A0, and A1 as the LDS-tiled scan (k_associate), the hashed grid (k_grid_count, the
4096-wide k_grid_scan with its carry, k_grid_fill, the nine-bucket query of k_associate_grid_dev) and the frame kernel's stride of 256 threads
with the min-reduction (k_frame_frontend).  It proves nothing about the device; it shows that the cases of frontend_shapes.py and the checker
of frontend_exact_ref.py catch the mistakes such kernels are prone to.  bugs: a set of planted mistakes,
    "le"            <= for < against the threshold                       (all three)
    "trunc"         truncation for floor in grid_coord, cones and queries alike — HARMLESS by itself: truncation is monotone and
                    trunc(a + 1) <= trunc(a) + 1, so cells only get wider and the 3 x 3 neighbourhood still covers the threshold
    "trunc_query"   truncation in the query's cell only, floor in the build (the one-sided form, which is a real mistake)
    "no_diag"       the neighbourhood without its four diagonal cells    (grid)
    "nearest"       the nearest match in place of the lowest index       (all three)
    "no_carry"      the scan starts every 4096-bucket pass at zero       (grid)
    "overwrite"     `found` overwritten by a later tile                  (tiled)
    "type_nofabs"   the type test without fabs                           (all three; what the frame kernel does ON PURPOSE with signed_type = 1)
    "sign_nofabs"   A0's sign = az / az                                  (polar_to_xy)
    "count_nonfinite"  non-finite map cones counted but not filled: their slots keep whatever they held; a query that reads one returns
                    UNINIT (-2), which no checker admits                 (grid)
Distances are numpy's dx * dx + dy * dy without contraction: a device that fuses the multiply-add may differ in the last place, which only a
pair inside the checker's band can show."""
import numpy as np

K_PIF = float(np.float32(3.14159265))
K_D2R = 0.017453292522222
K_R2D = 57.295779513082325
TILE = 1024
UNINIT = -2
BIG = 0x7fffffff


def polar_to_xy(az, zen, dist, lidar, bugs=()):
    az, zen, dist = (np.asarray(a, dtype=np.float64) for a in (az, zen, dist))
    with np.errstate(all="ignore"):
        sign = az / (az if "sign_nofabs" in bugs else np.abs(az))
        ang = K_PIF - np.abs(az * K_D2R)
        sa, ca = np.sin(ang), np.cos(ang)
        dnew = np.sqrt(lidar * lidar + dist * dist - 2.0 * lidar * dist * ca)
        az2 = np.arcsin((sa * dist) / dnew) * K_R2D * sign
        cz = np.cos(zen * K_D2R)
        return np.stack([dnew * cz * np.cos(az2 * K_D2R), dnew * cz * np.sin(az2 * K_D2R)], axis=-1)


def cone_to_global(poses, pose_of, obs, lidar, bugs=()):
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)[np.asarray(pose_of, dtype=np.int64)]
    obs = np.asarray(obs, dtype=np.float64).reshape(-1, 4)
    z = polar_to_xy(obs[:, 0], obs[:, 1], obs[:, 2], lidar, bugs)
    c, s = np.cos(poses[:, 2]), np.sin(poses[:, 2])
    with np.errstate(all="ignore"):
        return np.stack([(z[:, 0] * c - z[:, 1] * s) + poses[:, 0], (z[:, 0] * s + z[:, 1] * c) + poses[:, 1]], axis=-1)


def _pairs(gx, gy, ty, mx, my, mt, thr, tol, bugs, signed=False):
    """the pair test of one query against an array of cones: (matches, distances)"""
    with np.errstate(all="ignore"):
        if signed:
            ok = (mt - int(ty)).astype(np.float64) < tol
        elif "type_nofabs" in bugs:
            ok = (mt.astype(np.float64) - ty) < tol
        else:
            ok = np.abs(mt.astype(np.float64) - ty) < tol
        dx, dy = mx - gx, my - gy
        d = np.sqrt(dx * dx + dy * dy)
        return ok & ((d <= thr) if "le" in bugs else (d < thr)), d


def tiled(gxy, ty, map_xy, map_type, thr, tol, bugs=()):
    """k_associate: the map in tiles of 1024 through LDS, every query keeps its first match"""
    map_xy = np.asarray(map_xy, dtype=np.float64).reshape(-1, 2); map_type = np.asarray(map_type, dtype=np.int64)
    out = np.full(len(gxy), -1, dtype=np.int64)
    for i in range(len(gxy)):
        found = -1; best = np.inf
        for base in range(0, len(map_xy), TILE):
            if found >= 0 and "overwrite" not in bugs and "nearest" not in bugs:
                continue
            sl = slice(base, min(base + TILE, len(map_xy)))
            hit, d = _pairs(gxy[i, 0], gxy[i, 1], ty[i], map_xy[sl, 0], map_xy[sl, 1], map_type[sl], thr, tol, bugs)
            if hit.any():
                if "nearest" in bugs:
                    t = int(np.where(hit, d, np.inf).argmin())
                    if d[t] < best:
                        best = d[t]; found = base + t
                else:
                    found = base + int(hit.argmax())
        out[i] = found
    return out


def grid_coord(v, inv_cell, trunc=False):
    with np.errstate(all="ignore"):
        c = v * inv_cell
        c = np.trunc(c) if trunc else np.floor(c)
        c = np.fmin(np.fmax(c, -4.0e15), 4.0e15)                 # fmax / fmin drop a NaN: it lands on -4e15
        return np.where(np.isnan(c), -4.0e15, c).astype(np.int64)


def grid_bucket(cx, cy, mask):
    cx = np.asarray(cx, dtype=np.int64) & 0xffffffff; cy = np.asarray(cy, dtype=np.int64) & 0xffffffff
    return (((cx * 73856093) & 0xffffffff) ^ ((cy * 19349663) & 0xffffffff)) & mask


def buckets_of(n_map):
    b = 4096
    while b < 4 * n_map:
        b <<= 1
    return b


def inv_cell_of(thr):
    return 1.0 / (thr * (1.0 + 1e-9))


def grid_build(map_xy, thr, bugs=()):
    """count, scan (passes of 4096 buckets: 1024 threads x 4, with the carry), fill: (start [B + 1], items [n_map], inv_cell, mask)"""
    map_xy = np.asarray(map_xy, dtype=np.float64).reshape(-1, 2); n_map = len(map_xy)
    B = buckets_of(n_map); mask = B - 1; inv = inv_cell_of(thr); tr = "trunc" in bugs
    fin = np.isfinite(map_xy).all(axis=1)
    bk = grid_bucket(grid_coord(map_xy[:, 0], inv, tr), grid_coord(map_xy[:, 1], inv, tr), mask)
    count = np.zeros(B + 1, dtype=np.int64)
    np.add.at(count, bk if "count_nonfinite" in bugs else bk[fin], 1)
    start = np.zeros(B + 1, dtype=np.int64); carry = 0
    for base in range(0, B, 4096):
        v = count[base:base + 4096].reshape(-1, 4)               # four consecutive buckets per thread
        tsum = v.sum(axis=1)
        incl = np.cumsum(tsum)                                   # the wave scans and the sum over the waves before
        pre = 0 if "no_carry" in bugs else carry
        run = pre + incl - tsum
        for k in range(4):
            start[base + k:base + 4096:4] = run; run = run + v[:, k]
        carry = pre + int(incl[-1])
    start[B] = carry
    items = np.full(n_map, UNINIT, dtype=np.int64); cursor = np.zeros(B + 1, dtype=np.int64)
    for j in np.flatnonzero(fin):
        c = bk[j]
        q = start[c] + cursor[c]; cursor[c] += 1
        if 0 <= q < n_map:                                       # (a dropped carry makes passes share slots: the later cone wins, as a race would)
            items[q] = j
    return start, items, inv, mask


def grid(gxy, ty, map_xy, map_type, thr, tol, bugs=()):
    """k_associate_grid_dev over grid_build: nine buckets, the lowest matching index"""
    map_xy = np.asarray(map_xy, dtype=np.float64).reshape(-1, 2); map_type = np.asarray(map_type, dtype=np.int64)
    start, items, inv, mask = grid_build(map_xy, thr, bugs)
    tr = "trunc" in bugs or "trunc_query" in bugs
    out = np.full(len(gxy), -1, dtype=np.int64)
    for i in range(len(gxy)):
        gx, gy = gxy[i]
        if not (np.isfinite(gx) and np.isfinite(gy)):
            continue
        cx, cy = int(grid_coord(gx, inv, tr)), int(grid_coord(gy, inv, tr))
        found = BIG; best = np.inf
        for k in range(9):
            ox, oy = k % 3 - 1, k // 3 - 1
            if "no_diag" in bugs and ox and oy:
                continue
            b = int(grid_bucket(cx + ox, cy + oy, mask))
            js = items[start[b]:start[b + 1]]
            if not len(js):
                continue
            if (js == UNINIT).any():
                found = UNINIT; break
            hit, d = _pairs(gx, gy, ty[i], map_xy[js, 0], map_xy[js, 1], map_type[js], thr, tol, bugs)
            if hit.any():
                if "nearest" in bugs:
                    t = int(np.where(hit, d, np.inf).argmin())
                    if d[t] < best:
                        best = d[t]; found = int(js[t])
                else:
                    found = min(found, int(js[hit].min()))
        out[i] = -1 if found == BIG else found
    return out


def frame(gxy, ty, map_xy, map_type, thr, tol, signed=False, bugs=()):
    """k_frame_frontend: a workgroup per observation, thread tid takes j = tid, tid + 256, ... and stops at its first hit; the minimum over
    the 256 threads (wave shuffles, then four partial results through LDS)"""
    map_xy = np.asarray(map_xy, dtype=np.float64).reshape(-1, 2); map_type = np.asarray(map_type, dtype=np.int64); m = len(map_xy)
    rounds = (m + 255) // 256
    out = np.full(len(gxy), -1, dtype=np.int64)
    for i in range(len(gxy)):
        if m == 0:
            continue
        hit, d = _pairs(gxy[i, 0], gxy[i, 1], ty[i], map_xy[:, 0], map_xy[:, 1], map_type, thr, tol, bugs, signed)
        if "nearest" in bugs:
            out[i] = int(np.where(hit, d, np.inf).argmin()) if hit.any() else -1
            continue
        h = np.zeros(rounds * 256, dtype=bool); h[:m] = hit; h = h.reshape(rounds, 256)
        first = np.where(h.any(axis=0), h.argmax(axis=0) * 256 + np.arange(256), BIG)       # per thread: its first hit
        waves = first.reshape(4, 64).min(axis=1)
        found = int(waves.min())
        out[i] = -1 if found == BIG else found
    return out


ALL_BUGS = ("le", "trunc", "trunc_query", "no_diag", "nearest", "no_carry", "overwrite", "type_nofabs", "sign_nofabs", "count_nonfinite")
APPLIES = dict(le=("tiled", "grid", "frame"), trunc=("grid",), trunc_query=("grid",), no_diag=("grid",), nearest=("tiled", "grid", "frame"),
               no_carry=("grid",), overwrite=("tiled",), type_nofabs=("tiled", "grid", "frame"), sign_nofabs=("tiled", "grid", "frame"),
               count_nonfinite=("grid",))


def run(algo, poses, pose_of, obs, lidar, map_xy, map_type, thr, tol, bugs=(), signed=False, gxy=None):
    """one algorithm end to end (A0 in numpy unless gxy is given); thr <= 0 or NaN and an empty map take the tiled scan, as the host does"""
    obs = np.asarray(obs, dtype=np.float64).reshape(-1, 4)
    if gxy is None:
        gxy = cone_to_global(poses, pose_of, obs, lidar, bugs)
    if algo == "frame":
        return frame(gxy, obs[:, 3], map_xy, map_type, thr, tol, signed, bugs)
    if algo == "grid" and len(np.asarray(map_xy).reshape(-1, 2)) > 0 and thr > 0:
        return grid(gxy, obs[:, 3], map_xy, map_type, thr, tol, bugs)
    return tiled(gxy, obs[:, 3], map_xy, map_type, thr, tol, bugs)
