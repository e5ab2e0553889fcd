"""The reference of the cone candidates (TEST-ONLY), written from include/graphslam.h ("cone candidates") — not from the kernels.

DECISIONS.  Which slot an observation takes is the association's answer (the tests hold it bitwise to gs_assign_opt_batch over the device's own
table); given slot and n_admissible per observation, everything else of a step that is an integer — who fuses, who is contested, far, spawns
or is dropped, spawn ranks and slots, ids, hits, misses, states, retirement, confirmation, every counter, next_id and t — is repeated by
`advance` and held BIT FOR BIT.  The spawn-range test compares two inputs (the distance column and spawn_range): it has no band.

VALUES.  The fused l+, C+ and the spawned xy, cov are carried as assoc_nn_ref.E pairs (exact value in mpmath, first-order error e) by that
module's rules, starting from assoc_nn_ref.Query's g and A = Q + P and from the table before the step, whose fp64 numbers are taken exactly:
    S = C + A         addition 1 each                                                   sum rule
    det = S00 S11 - S01 S01            products 1, subtraction 1                        product and sum rules (the cancellation of assoc_nn_ref)
    n = g - l         subtraction 1                                                     sum rule
    K00 = (C00 S11 - C01 S01) / det    products 1, subtraction 1, division 1            (K01, K10, K11 likewise)
    DIVISION RULE   q = a / b:  e = (e_a + |q| e_b) / (|b| - 2 e_b) + u |q|             (the rule assoc_nn_ref states for k and d2)
    l+ = l + (K00 n0 + K01 n1)         products 1, additions 2
    C+ = K A          products 1, addition 1 each; the 01 entry once
    product rule   e(a b) = |a| e_b + |b| e_a + u |a b|;   sum rule   e(a + b) = e_a + e_b + u |a + b|;   B = 2 e (the total doubled)
u = 2^-53.  A spawned slot's xy and cov are the query's g and A themselves: held to THEIR e.  REFUSALS (assertions, where first order ends):
2 e_det <= 1e-6 |det| for every fusion.  Nothing here is fitted to a device output.

VISIBILITY rests on a sincos: (s, c) = sincos(theta) with e = 4 u |.| as frontend_exact_ref counts the device's; ex = lx - tx, ey = ly - ty,
dx = c ex + s ey, dy = c ey - s ex, r2 = dx dx + dy dy as E pairs.  The range test r2 < view2 (view2 = the fp64 product view_range view_range,
an input) has the band 2 e_r2; the cone test dx >= view_cos sqrt(r2) has the band 2 (e_dx + e_m), m = view_cos sqrt(r2) with the sqrt
correctly rounded (e = e_r2 / (2 sqrt) + u sqrt).  A scene in which a test that decides falls inside its band is REJECTED (class Rejected):
it cannot be held bit for bit, and no case may be skipped — the scenes are built with margin and test_cand_cpu asserts none is rejected.
Two exact cases need no band: view_cos == -1 (all-round) is true for every finite d, because fl(sqrt(fl(fl(dx dx) + fl(dy dy)))) >= |dx| for
correctly rounded operations (sqrt(fl(x x)) = |x| and rounding is monotone); and l == t gives dx = r2 = 0, where 0 >= view_cos 0 holds.

THE REPLAY (`replay`) runs whole sequences in plain float64 for the CPU tests: the query, d2 and the fusion by the header's lines with one
ufunc per operation (`F64`), the association as a small exact search — every observation's admissible slots, connected groups of observations
that share slots, the matching of largest total gain inside a group by enumeration; it REFUSES a group above 7 observations, more than
GS_ASSIGN_CAND_MAX admissible slots and a tie — and `advance`.  It records the smallest margin by which a gate, Euclidean or visibility
decision was taken (`margins`), which test_cand_cpu holds above 1e-6: a thousand million times the rounding of either side."""
import numpy as np

import assoc_exec as ax
import assoc_nn_ref as nr
import frontend_exact_ref as fx

E, U, MP, mpf = nr.E, nr.U, nr.MP, nr.mpf
CAND_MAX = 1024
FRAME_MAX = 256
ASSIGN_CAND_MAX = 8
FREE, TENTATIVE, CONFIRMED = 0, 1, 2
CAND = np.dtype([("xy", "<f8", 2), ("cov", "<f8", 4), ("type", "<i4"), ("id", "<i4"), ("state", "<i4"), ("hits", "<i4"), ("misses", "<i4"),
                 ("first_step", "<i4"), ("last_step", "<i4"), ("confirm_step", "<i4")])
STEP_KEYS = ("step", "n_unexplained", "n_fused", "n_spawned", "n_contested", "n_far", "n_dropped", "n_missed", "n_retired", "n_confirmed", "n_live")
INT_KEYS = ("type", "id", "state", "hits", "misses", "first_step", "last_step", "confirm_step")
DEFAULTS = dict(confirm_hits=3, max_misses=3, spawn_range=67.0, view_range=12.0, view_cos=0.5)


class Rejected(AssertionError):
    """a decision of the scene falls inside its band: the scene cannot be held bit for bit"""


def params_of(**kw):
    p = dict(DEFAULTS); p.update(kw)
    return p


# ---- the table
def free_record():
    r = np.zeros((), dtype=CAND); r["xy"] = np.nan; r["id"] = -1; r["confirm_step"] = -1
    return r


def record(xy, cov=(0.04, 0.0, 0.0, 0.04), type=1, id=0, state=TENTATIVE, hits=1, misses=0, first_step=0, last_step=0, confirm_step=-1):
    r = np.zeros((), dtype=CAND)
    r["xy"] = xy; r["cov"] = cov; r["type"] = type; r["id"] = id; r["state"] = state; r["hits"] = hits; r["misses"] = misses
    r["first_step"] = first_step; r["last_step"] = last_step; r["confirm_step"] = confirm_step
    return r


def load(records=None):
    """(table [CAND_MAX], meta = [next_id, t, n_live]) as loading `records` leaves it: record s in slot s as it is, state 0 a free slot, the
    rest free; next_id = 1 + the largest id, t = 1 + the largest last_step over the loaded records that are not free, 0 without one"""
    tab = np.empty(CAND_MAX, dtype=CAND); tab[:] = free_record()
    rec = np.zeros(0, dtype=CAND) if records is None else np.asarray(records, dtype=CAND).reshape(-1)
    assert len(rec) <= CAND_MAX
    live = [s for s in range(len(rec)) if rec[s]["state"] in (TENTATIVE, CONFIRMED)]
    for s in live:
        tab[s] = rec[s]
    meta = [1 + max(int(tab[s]["id"]) for s in live), 1 + max(int(tab[s]["last_step"]) for s in live), len(live)] if live else [0, 0, 0]
    return tab, meta


def as_map(tab):
    """the table as the association takes it: (xy [1024, 2], type [1024], cov [1024, 4])"""
    return np.ascontiguousarray(tab["xy"]), np.ascontiguousarray(tab["type"]), np.ascontiguousarray(tab["cov"])


def masked(frame, in_idx):
    """the frame with the azimuth of every explained observation replaced by NaN"""
    ob = np.array(frame, dtype=np.float64).reshape(-1, 4)
    if in_idx is not None:
        ob[np.asarray(in_idx).reshape(-1) >= 0, 0] = np.nan
    return ob


# ---- the integer side of a step (bit for bit)
def advance(tab, meta, frame, in_idx, slot, na, valid, visible, cp):
    """one step's decisions.  tab, meta: before the step (not changed).  slot, na: the association's answer per observation; valid[i]: the
    query of observation i is valid; visible(s): slot s is visible from the step's pose (asked only for slots the rule asks about).
    Returns (table after — the VALUES of fused and spawned slots still to be written —, meta after, step record, cand_id, cand_slot,
    fused [(i, c)], spawned [(i, s)])"""
    frame = np.asarray(frame, dtype=np.float64).reshape(-1, 4); k = len(frame)
    assert k <= FRAME_MAX
    out = tab.copy(); next_id, t, _ = (int(v) for v in meta)
    in_u = np.ones(k, dtype=bool) if in_idx is None else np.asarray(in_idx).reshape(-1) < 0
    fused, spawners, n_cont, n_far = [], [], 0, 0
    for i in range(k):
        if not (in_u[i] and valid[i]):
            continue
        c = int(slot[i])
        if 0 <= c < CAND_MAX:
            fused.append((i, c))
        elif int(na[i]) > 0:
            n_cont += 1
        elif frame[i, 2] < cp["spawn_range"]:
            spawners.append(i)
        else:
            n_far += 1
    assert len({c for _, c in fused}) == len(fused), "the association gave one slot to two observations"
    was_free = [s for s in range(CAND_MAX) if tab[s]["state"] == FREE]
    hit = {c for _, c in fused}
    n_missed = n_retired = n_confirmed = 0
    for s in range(CAND_MAX):
        st = int(tab[s]["state"])
        if st == FREE:
            continue
        if s in hit:
            out["hits"][s] += 1; out["misses"][s] = 0; out["last_step"][s] = t
        elif visible(s):
            n_missed += 1
            if st == TENTATIVE and int(tab[s]["misses"]) + 1 >= cp["max_misses"]:
                out[s] = free_record(); n_retired += 1; st = FREE
            else:
                out["misses"][s] += 1
        if st == TENTATIVE and int(out["hits"][s]) >= cp["confirm_hits"]:
            out["state"][s] = CONFIRMED; out["confirm_step"][s] = t; n_confirmed += 1
    taken = min(len(spawners), len(was_free)); spawned = []
    cid = np.full(k, -1, dtype=np.int32); cslot = np.full(k, -1, dtype=np.int32)
    for i, c in fused:
        cid[i] = tab[c]["id"]; cslot[i] = c
    now = cp["confirm_hits"] <= 1
    for r in range(taken):
        i, s = spawners[r], was_free[r]
        ty = frame[i, 3]; ty = int(np.clip(np.trunc(ty), -2 ** 31, 2 ** 31 - 1)) if np.isfinite(ty) else 0
        out["type"][s] = ty; out["id"][s] = next_id + r; out["state"][s] = CONFIRMED if now else TENTATIVE; out["hits"][s] = 1; out["misses"][s] = 0
        out["first_step"][s] = t; out["last_step"][s] = t; out["confirm_step"][s] = t if now else -1
        cid[i] = next_id + r; cslot[i] = s; spawned.append((i, s))
    n_live = int((tab["state"] != FREE).sum()) - n_retired + taken
    rec = dict(step=t, n_unexplained=int(in_u.sum()), n_fused=len(fused), n_spawned=taken, n_contested=n_cont, n_far=n_far, n_dropped=len(spawners) - taken,
               n_missed=n_missed, n_retired=n_retired, n_confirmed=n_confirmed + (taken if now else 0), n_live=n_live)
    return out, [next_id + taken, t + 1, n_live], rec, cid, cslot, fused, spawned


# ---- float64: one ufunc per operation, the header's order
f8 = np.float64


def query64(pose, pc, ob, lidar, p):
    """the query of one observation in float64: dict(valid, g [2], A [3] = a00 a01 a11)"""
    with np.errstate(all="ignore"):
        z = ax.polar_to_xy(ob[0], ob[1], ob[2], lidar); zx, zy = f8(z[0]), f8(z[1])
        c, s = np.cos(f8(pose[2])), np.sin(f8(pose[2]))
        wx = zx * c - zy * s; wy = zx * s + zy * c
        gx = wx + f8(pose[0]); gy = wy + f8(pose[1])
        r2 = zx * zx + zy * zy
        k = (f8(p["sigma_range"]) * f8(p["sigma_range"])) / r2; sb2 = f8(p["sigma_bearing"]) * f8(p["sigma_bearing"]); sx2 = f8(p["sigma_xy"]) * f8(p["sigma_xy"])
        a00 = ((k * wx) * wx + (sb2 * wy) * wy) + sx2
        a01 = (k * wx) * wy - (sb2 * wx) * wy
        a11 = ((k * wy) * wy + (sb2 * wx) * wx) + sx2
        if pc is not None:
            pc = np.asarray(pc, dtype=f8).reshape(9); ux, uy = -wy, wx
            a00 = a00 + ((pc[0] + (f8(2.0) * pc[2]) * ux) + (pc[8] * ux) * ux)
            a01 = a01 + (((pc[1] + pc[2] * uy) + pc[5] * ux) + (pc[8] * ux) * uy)
            a11 = a11 + ((pc[4] + (f8(2.0) * pc[5]) * uy) + (pc[8] * uy) * uy)
    return dict(valid=bool(np.isfinite(gx) and np.isfinite(gy) and r2 > 0.0), g=np.array([gx, gy]), A=np.array([a00, a01, a11]), ty=float(ob[3]))


def pair64(q, l, C, ty, p):
    """(admissible, d2, the smallest relative margin of its Euclidean and gate tests) of a slot against a query, in float64"""
    with np.errstate(all="ignore"):
        if not abs(float(ty) - q["ty"]) < p["type_tol"]:
            return False, np.inf, np.inf
        n0 = f8(l[0]) - q["g"][0]; n1 = f8(l[1]) - q["g"][1]
        eu = np.sqrt(n0 * n0 + n1 * n1)
        s00 = f8(C[0]) + q["A"][0]; s01 = f8(C[1]) + q["A"][1]; s11 = f8(C[3]) + q["A"][2]
        det = s00 * s11 - s01 * s01
        d2 = (((s11 * n0) * n0 - ((f8(2.0) * s01) * n0) * n1) + (s00 * n1) * n1) / det
        if not np.isfinite(eu):
            return False, np.inf, np.inf
        m = abs(eu - p["max_distance"]) / p["max_distance"]
        if not eu < p["max_distance"]:
            return False, np.inf, m
        if not (det > 0.0 and s00 > 0.0):
            return False, np.inf, m
        m = min(m, abs(d2 - p["gate_chi2"]) / p["gate_chi2"])
        return bool(d2 < p["gate_chi2"]), float(d2), m


def _fuse(l, C, g, A, div):
    """the header's fusion lines over any arithmetic: l, C (00 01 11), g, A (00 01 11) -> (lx+, ly+, C00+, C01+, C11+)"""
    s00 = C[0] + A[0]; s01 = C[1] + A[1]; s11 = C[2] + A[2]
    det = (s00 * s11) - (s01 * s01)
    n0 = g[0] - l[0]; n1 = g[1] - l[1]
    k00 = div((C[0] * s11) - (C[1] * s01), det); k01 = div((C[1] * s00) - (C[0] * s01), det)
    k10 = div((C[1] * s11) - (C[2] * s01), det); k11 = div((C[2] * s00) - (C[1] * s01), det)
    return (l[0] + ((k00 * n0) + (k01 * n1)), l[1] + ((k10 * n0) + (k11 * n1)),
            (k00 * A[0]) + (k01 * A[1]), (k00 * A[1]) + (k01 * A[2]), (k10 * A[1]) + (k11 * A[2]))


def fuse64(l, cov4, g, A):
    with np.errstate(all="ignore"):
        return _fuse([f8(l[0]), f8(l[1])], [f8(cov4[0]), f8(cov4[1]), f8(cov4[3])], [f8(g[0]), f8(g[1])], [f8(a) for a in A], lambda a, b: a / b)


def div_exact(a, b):
    """the division rule of the module docstring"""
    assert 2 * b.e <= mpf(1e-6) * abs(b.v), ("S is too close to singular for a first-order bound", float(b.v), float(b.e))
    q = a.v / b.v
    return E(q, (a.e + abs(q) * b.e) / (abs(b.v) - 2 * b.e) + U * abs(q))


def fuse_exact(l, cov4, q):
    """the fusion of an assoc_nn_ref.Query with a slot (its numbers taken exactly) as five E pairs"""
    return _fuse([E(l[0]), E(l[1])], [E(cov4[0]), E(cov4[1]), E(cov4[3])], [q.gx, q.gy], [q.a00, q.a01, q.a11], div_exact)


def inside(dev, ref):
    """|dev - exact| <= B = 2 e, and how much of B it takes (0 where both are exact and equal)"""
    d = abs(mpf(float(dev)) - ref.v); B = 2 * ref.e
    return d <= B, (float(d / B) if B > 0 else (0.0 if d == 0 else float("inf")))


def visible64(l, pose, cp, margins=None):
    with np.errstate(all="ignore"):
        c, s = np.cos(f8(pose[2])), np.sin(f8(pose[2]))
        ex = f8(l[0]) - f8(pose[0]); ey = f8(l[1]) - f8(pose[1])
        dx = (c * ex) + (s * ey); dy = (c * ey) - (s * ex)
        r2 = (dx * dx) + (dy * dy); v2 = f8(cp["view_range"]) * f8(cp["view_range"])
        if not np.isfinite(r2):
            return False
        if margins is not None:
            margins.append(abs(r2 - v2) / v2)
        if not r2 < v2:
            return False
        m = f8(cp["view_cos"]) * np.sqrt(r2)
        if margins is not None and cp["view_cos"] != -1.0 and r2 > 0:
            margins.append(abs(dx - m) / np.sqrt(r2))
        return bool(dx >= m)


def visible_exact(l, pose, cp):
    """the visibility of a slot with its bands; raises Rejected where a deciding test falls inside its band"""
    if not (np.isfinite(l).all() and np.isfinite(pose).all()):
        return False
    th = mpf(float(pose[2])); cv, sv = MP.cos(th), MP.sin(th)
    c = E(cv, 4 * U * abs(cv)); s = E(sv, 4 * U * abs(sv))
    ex = E(l[0]) - E(pose[0]); ey = E(l[1]) - E(pose[1])
    dx = (c * ex) + (s * ey); dy = (c * ey) - (s * ex)
    r2 = (dx * dx) + (dy * dy)
    v2 = mpf(float(f8(cp["view_range"]) * f8(cp["view_range"])))
    if ex.v == 0 and ey.v == 0:
        return bool(0 < v2)
    if abs(r2.v - v2) <= 2 * r2.e:
        raise Rejected("the range test of a slot at (%g, %g) falls inside its band" % (l[0], l[1]))
    if not r2.v < v2:
        return False
    if cp["view_cos"] == -1.0:
        return True
    sq = MP.sqrt(r2.v); m = E(cp["view_cos"]) * E(sq, r2.e / (2 * sq) + U * sq)
    if abs(dx.v - m.v) <= 2 * (dx.e + m.e):
        raise Rejected("the cone test of a slot at (%g, %g) falls inside its band" % (l[0], l[1]))
    return bool(dx.v > m.v)


# ---- the checker of one device step
class StepCheck:
    """what one step of a device run must be, from the device's own table before it and the association's answer"""

    def __init__(self, before, meta, frame, in_idx, pose, pose_cov, slot, na, prm, cp, lidar):
        frame = np.asarray(frame, dtype=np.float64).reshape(-1, 4); k = len(frame); pose = np.asarray(pose, dtype=np.float64).reshape(3)
        self.k = k; self.q = {}
        in_u = np.ones(k, dtype=bool) if in_idx is None else np.asarray(in_idx).reshape(-1) < 0
        valid = np.zeros(k, dtype=bool)
        if k and np.isfinite(pose).all():
            R = fx.Ref(frame, pose.reshape(1, 3), np.zeros(k, dtype=np.int64), lidar)
            for i in np.flatnonzero(in_u):
                if R.nan[i]:
                    continue
                if R.band[i]:
                    raise Rejected("observation %d is in A0's branch band" % i)
                q = nr.Query(R, int(i), pose, pose_cov, prm)
                if q.valid:
                    assert MP.isfinite(q.gx.v) and MP.isfinite(q.gy.v)
                    valid[i] = True; self.q[int(i)] = q
        self.valid = valid
        self.after, self.meta, self.rec, self.cid, self.cslot, self.fused, self.spawned = advance(
            before, meta, frame, in_idx, slot, na, valid, lambda s: visible_exact(before[s]["xy"], pose, cp), cp)
        self.values = {}                                                       # slot -> (x, y, c00, c01, c11) as E pairs
        for i, c in self.fused:
            self.values[c] = fuse_exact(before[c]["xy"], before[c]["cov"], self.q[i])
        for i, s in self.spawned:
            q = self.q[i]; self.values[s] = (q.gx, q.gy, q.a00, q.a01, q.a11)

    def failures(self, after, meta, rec, cid, cslot):
        """[what] for everything of the device's step that is not what it must be; self.worst = the largest fraction of a bound reached"""
        bad = []; self.worst = 0.0
        if [int(v) for v in meta] != self.meta:
            bad.append(("meta", [int(v) for v in meta], self.meta))
        for key in STEP_KEYS:
            if int(rec[key]) != self.rec[key]:
                bad.append(("step record", key, int(rec[key]), self.rec[key]))
        if np.asarray(cid).tobytes() != self.cid.tobytes():
            bad.append(("cand_id", np.asarray(cid).tolist(), self.cid.tolist()))
        if np.asarray(cslot).tobytes() != self.cslot.tobytes():
            bad.append(("cand_slot", np.asarray(cslot).tolist(), self.cslot.tolist()))
        for s in range(CAND_MAX):
            if s not in self.values:
                if after[s].tobytes() != self.after[s].tobytes():
                    bad.append(("slot %d" % s, after[s], self.after[s]))
                continue
            for key in INT_KEYS:
                if int(after[s][key]) != int(self.after[s][key]):
                    bad.append(("slot %d" % s, key, int(after[s][key]), int(self.after[s][key])))
            if after[s]["cov"][1].tobytes() != after[s]["cov"][2].tobytes():
                bad.append(("slot %d" % s, "cov is not bitwise symmetric"))
            got = (after[s]["xy"][0], after[s]["xy"][1], after[s]["cov"][0], after[s]["cov"][1], after[s]["cov"][3])
            for what, dev, ref in zip(("x", "y", "c00", "c01", "c11"), got, self.values[s]):
                ok, ratio = inside(dev, ref)
                if not ok:
                    bad.append(("slot %d" % s, what, float(dev), float(ref.v), ratio))
                else:
                    self.worst = max(self.worst, ratio)
        return bad


# ---- the float64 replay of whole runs
def associate64(tab, pose, pc, frame, in_idx, prm, lidar, margins):
    """(slot [k], n_admissible [k], valid [k], queries): the minimum-cost association of the unexplained observations against the table"""
    frame = np.asarray(frame, dtype=np.float64).reshape(-1, 4); k = len(frame)
    in_u = np.ones(k, dtype=bool) if in_idx is None else np.asarray(in_idx).reshape(-1) < 0
    slot = np.full(k, -1, dtype=np.int32); na = np.zeros(k, dtype=np.int32); valid = np.zeros(k, dtype=bool); qs = {}; cand = {}
    live = [s for s in range(CAND_MAX) if tab[s]["state"] != FREE]
    for i in np.flatnonzero(in_u):
        q = query64(pose, pc, frame[i], lidar, prm)
        if not q["valid"]:
            continue
        valid[i] = True; qs[int(i)] = q; lst = []
        for s in live:
            ok, d2, m = pair64(q, tab[s]["xy"], tab[s]["cov"], tab[s]["type"], prm)
            if np.isfinite(m):
                margins.append(m)
            if ok:
                lst.append((d2, s))
        na[i] = len(lst)
        assert len(lst) <= ASSIGN_CAND_MAX, "the replay refuses more than GS_ASSIGN_CAND_MAX admissible slots"
        if lst:
            cand[int(i)] = sorted(lst)
    todo = set(cand)
    while todo:                                                                # groups of observations that share slots
        grp = {todo.pop()}; grew = True
        while grew:
            grew = False; slots = {s for i in grp for _, s in cand[i]}
            for j in list(todo):
                if slots & {s for _, s in cand[j]}:
                    grp.add(j); todo.discard(j); grew = True
        grp = sorted(grp)
        assert len(grp) <= 7, "the replay refuses a group of more than 7 contending observations"
        best = [(-1.0, None)]; second = [-1.0]

        def walk(pos, used, gain, pick):
            if pos == len(grp):
                if gain > best[0][0]:
                    second[0] = best[0][0]; best[0] = (gain, dict(pick))
                elif gain > second[0]:
                    second[0] = gain
                return
            i = grp[pos]
            walk(pos + 1, used, gain, pick)
            for d2, s in cand[i]:
                if s not in used:
                    pick[i] = s; walk(pos + 1, used | {s}, gain + (prm["gate_chi2"] - d2), pick); del pick[i]
        walk(0, frozenset(), 0.0, {})
        assert best[0][0] - second[0] > 1e-9 * prm["gate_chi2"] or len(grp) == 1, "the replay refuses a tie between two matchings"
        for i, s in best[0][1].items():
            slot[i] = s
    return slot, na, valid, qs


def replay(records, poses, pose_covs, frames, in_idxs, prm, cp, lidar):
    """a whole run in float64 from the loaded records: dict(steps, cand_id [per frame], cand_slot, table, meta, margins, tables = the table after
    every step)"""
    tab, meta = load(records); steps, ids, slots, tables, margins = [], [], [], [], []
    for t, frame in enumerate(frames):
        pose = np.asarray(poses[t], dtype=np.float64); pc = None if pose_covs is None else pose_covs[t]; ii = None if in_idxs is None else in_idxs[t]
        slot, na, valid, qs = associate64(tab, pose, pc, frame, ii, prm, lidar, margins)
        before = tab
        tab, meta, rec, cid, cslot, fused, spawned = advance(before, meta, frame, ii, slot, na, valid, lambda s: visible64(before[s]["xy"], pose, cp, margins), cp)
        for i, c in fused:
            x, y, c00, c01, c11 = fuse64(before[c]["xy"], before[c]["cov"], qs[i]["g"], qs[i]["A"])
            tab["xy"][c] = (x, y); tab["cov"][c] = (c00, c01, c01, c11)
        for i, s in spawned:
            a = qs[i]["A"]; tab["xy"][s] = qs[i]["g"]; tab["cov"][s] = (a[0], a[1], a[1], a[2])
        steps.append(rec); ids.append(cid); slots.append(cslot); tables.append(tab.copy())
    return dict(steps=steps, cand_id=ids, cand_slot=slots, table=tab, meta=meta, margins=margins, tables=tables)
