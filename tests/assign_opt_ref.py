"""The minimum-cost association inside a frame (TEST-ONLY), written from include/graphslam.h ("minimum-cost association") — not from the kernel.

A frame is `rows`: per observation the list of its admissible pairs (d2, cone).  cut() keeps the GS_ASSIGN_CAND_MAX = 8 smallest by (d2, cone).
Over the cut lists the rule asks for a matching of largest total gain sum(gate - d2); it is stated twice, both in EXACT arithmetic (every
number — a float, an mpmath number, a Fraction — is a dyadic rational; a frame is brought to one common power-of-two denominator and solved
in Python integers):
    enumerate_best   every matching of a small frame, by recursion over the observations
    solve            successive shortest augmenting paths: the observations one after the other, each by Dijkstra over reduced costs with a
                     private dummy column of cost `gate`; connected components of the frame are solved one by one
margin() is the distance from the best total to the best total of any DIFFERENT matching: a different matching drops at least one optimal
pair, so it is the smallest, over the optimal pairs, of best - best(with that pair forbidden).

THE TOLERANCE T(k) = 48 k^2 u gate, u = 2^-53 (DESIGN §24 has the same count).  The device solves with fp64 duals: u_i per observation, v_j per
cone, both in [0, gate] in magnitude, tree distances rd <= gate, d2 < gate.  Per augmentation a dual changes once.  What can move the slack
c - u_i - v_j of one pair in one augmentation:  the key ((rd + d2) - u) - v, three roundings of results below 2, 2 and 3 gate: 7 u gate;
the step delta = min - rd, a result below gate, once for each end of the pair: 2 u gate;  u += delta and v -= delta, results below 2 gate:
4 u gate.  13 u gate, counted as 16.  After k augmentations every slack is within 16 k u gate of what exact duals would give (the roundings
add, they do not multiply: a tree distance enters the key and the delta as the same stored number).  A matching whose pairs have slack <= s and
whose other pairs have slack >= -s, with v <= s, is within 3 k s of the optimum: T = 3 k * 16 k u gate.  Nothing here is measured on a device.

DECIDED.  A frame is DECIDED when (a) every candidate pair is surely admissible or surely not, (b) where an observation has more than 8
admissible cones the 8th and the 9th by d2 have disjoint intervals [d2 - B, d2 + B], and (c) margin >= 1000 (T + 2 sum B), the sum over the
frame's cut pairs (a matching's total moves by at most sum B when every d2 moves by its B; 1000 is headroom for the derivation of T).  Then the
device must return the exact optimum's indices.  Whatever the frame, a result must be a valid matching (no cone twice) of pairs that are
possibly admissible and possibly among their observation's 8 best, with d2 within the pair's B and n_admissible between the surely and the
possibly admissible counts, and it must be maximal: no observation at -1 while a cone surely on its list is free."""
from fractions import Fraction

import numpy as np

CAND_MAX = 8
INF = float("inf")
U = Fraction(1, 2 ** 53)
C_T = 48


def T(k, gate):
    return C_T * k * k * U * frac(gate)


def frac(x):
    """the exact value of a float, an int, a Fraction or an mpmath number"""
    if isinstance(x, Fraction):
        return x
    if isinstance(x, (int, np.integer)):
        return Fraction(int(x))
    if isinstance(x, (float, np.floating)):
        return Fraction(float(x))
    s, man, exp, _ = x._mpf_                                                 # mpmath: (-1)^s man 2^exp
    v = Fraction(int(man)) * (Fraction(2) ** int(exp))
    return -v if s else v


def rows_of(D, cones=None):
    """a distance matrix (+inf / None = not admissible) as rows of (d2, cone)"""
    k = len(D); m = len(D[0]) if k else 0
    cones = list(range(m)) if cones is None else list(cones)
    return [[(D[i][c], cones[c]) for c in range(m) if D[i][c] is not None and D[i][c] != INF] for i in range(k)]


def cut(rows, cap=CAND_MAX):
    return [sorted(r, key=lambda p: (frac(p[0]), p[1]))[:cap] for r in rows]


def _ints(rows, gate):
    """(integer rows, integer gate, scale): every d2 and the gate times one power of two"""
    fr = [[(frac(d), j) for d, j in r] for r in rows]; g = frac(gate)
    den = max([g.denominator] + [d.denominator for r in fr for d, _ in r])
    assert all(den % d.denominator == 0 for r in fr for d, _ in r) and den % g.denominator == 0      # (powers of two)
    return [[(int(d * den), j) for d, j in r] for r in fr], int(g * den), den


def value(rows, idx, gate):
    """the total gain of the matching idx (cone or -1 per observation) as a Fraction; asserts that it is a matching over the rows' pairs"""
    tot = Fraction(0); used = set()
    for r, j in zip(rows, idx):
        if j == -1:
            continue
        assert j not in used, "cone %d twice" % j
        used.add(j)
        d = [d for d, c in r if c == j]; assert len(d) == 1, "pair (., %d) is not in the lists" % j
        tot += frac(gate) - frac(d[0])
    return tot


def enumerate_best(rows, gate):
    """(best total gain as a Fraction, one best matching) over ALL matchings of the (cut) rows: exponential, for small frames"""
    R, g, den = _ints(rows, gate); k = len(R); best = [-1, None]; cur = [-1] * k; used = set()
    def rec(i, tot):
        if i == k:
            if tot > best[0]:
                best[0] = tot; best[1] = list(cur)
            return
        cur[i] = -1; rec(i + 1, tot)
        for d, j in R[i]:
            if j not in used:
                used.add(j); cur[i] = j; rec(i + 1, tot + g - d); used.discard(j)
        cur[i] = -1
    rec(0, 0)
    return Fraction(best[0], den), best[1]


def _components(R):
    """the frame's observations grouped by shared cones: [[observation, ...]] in ascending order"""
    parent = list(range(len(R)))
    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]; a = parent[a]
        return a
    owner = {}
    for i, r in enumerate(R):
        for _, j in r:
            if j in owner:
                parent[find(i)] = find(owner[j])
            else:
                owner[j] = i
    comp = {}
    for i in range(len(R)):
        comp.setdefault(find(i), []).append(i)
    return sorted(comp.values())


def _ssp(R, g, members, forbid=None):
    """successive shortest paths over the observations `members` of the integer rows R; (total gain, {observation: cone})"""
    import heapq
    u = {}; v = {}; mate = {}; owner = {}                                    # duals; observation -> cone or ("d", i); cone -> observation
    def edges(i):
        for d, j in R[i]:
            if (i, j) != forbid:
                yield d, j
        yield g, ("d", i)
    for root in members:
        u[root] = 0; dist = {}; pred = {}; done = set(); heap = []; tree = {root: 0}; sink = None
        def relax(i, base):
            for d, j in edges(i):
                if j in done:
                    continue
                nd = base + d - u[i] - v.get(j, 0)
                if j not in dist or nd < dist[j]:
                    dist[j] = nd; pred[j] = i; heapq.heappush(heap, (nd, str(j), j))
        relax(root, 0)
        while True:
            nd, _, j = heapq.heappop(heap)
            if j in done or nd != dist[j]:
                continue
            done.add(j)
            if j not in owner:
                sink = j; low = nd
                break
            i = owner[j]; tree[i] = nd; relax(i, nd)
        for i, base in tree.items():
            u[i] += low - base
            if i != root:
                v[mate[i]] = v.get(mate[i], 0) - (low - base)
        j = sink
        while True:
            i = pred[j]; old = mate.get(i); mate[i] = j; owner[j] = i
            if i == root:
                break
            j = old
    tot = 0; out = {}
    for i in members:
        j = mate[i]
        if not isinstance(j, tuple):
            out[i] = j; tot += g - [d for d, c in R[i] if c == j][0]
    return tot, out


def solve(rows, gate):
    """(best total gain as a Fraction, the matching as cone or -1 per observation) of the (cut) rows, by successive shortest paths"""
    R, g, den = _ints(rows, gate); idx = [-1] * len(R); tot = 0
    for members in _components(R):
        t, m = _ssp(R, g, members); tot += t
        for i, j in m.items():
            idx[i] = j
    return Fraction(tot, den), idx


def margin(rows, gate):
    """best total minus the best total of any different matching (a Fraction; +inf for a frame without an admissible pair)"""
    R, g, den = _ints(rows, gate); worst = None
    for members in _components(R):
        best, m = _ssp(R, g, members)
        for i, j in m.items():
            gap = best - _ssp(R, g, members, forbid=(i, j))[0]
            assert gap >= 0
            worst = gap if worst is None else min(worst, gap)
    return INF if worst is None else Fraction(worst, den)


class FrameRef:
    """one frame against the exact reference R (assoc_nn_ref.Ref): members = the reference's observation numbers in the frame's order"""

    def __init__(self, R, members):
        self.R = R; self.members = [int(i) for i in members]; self.k = len(self.members); self.gate = R.p["gate_chi2"]
        self.pairs = {}; self.n_sure = []; self.n_poss = []; self.in_cut = {}; self.sure_in = {}
        undecided = False; rows = []; sum_b = 0
        for a, i in enumerate(self.members):
            cs = [cd for cd in R.cands[i] if cd.poss]
            undecided |= any(cd.poss != cd.sure for cd in R.cands[i])
            self.n_poss.append(len(cs)); self.n_sure.append(sum(cd.sure for cd in cs))
            cs.sort(key=lambda cd: (cd.d2, cd.j))
            if len(cs) > CAND_MAX and not cs[CAND_MAX - 1].d2 + cs[CAND_MAX - 1].B < cs[CAND_MAX].d2 - cs[CAND_MAX].B:
                undecided = True
            for cd in cs:
                self.pairs[(a, cd.j)] = cd
                surely_better = sum(1 for o in cs if o is not cd and o.sure and o.d2 + o.B < cd.d2 - cd.B)
                possibly_better = sum(1 for o in cs if o is not cd and o.d2 - o.B <= cd.d2 + cd.B)
                self.in_cut[(a, cd.j)] = surely_better < CAND_MAX                       # possibly among the 8 best
                self.sure_in[(a, cd.j)] = cd.sure and possibly_better < CAND_MAX        # surely on the list
            rows.append([(cd.d2, cd.j) for cd in cs[:CAND_MAX]]); sum_b += sum(frac(cd.B) for cd in cs[:CAND_MAX])
        self.rows = rows; self.sum_b = sum_b; self.T = T(self.k, self.gate)
        self.best, self.expect = solve(rows, self.gate)
        self.margin = margin(rows, self.gate)
        self.decided = not undecided and self.margin >= 1000 * (self.T + 2 * sum_b)

    def greedy(self):
        """the greedy matching in ascending (d2, observation, cone) over the same cut lists: (index, total gain)"""
        pairs = sorted((frac(d), a, j) for a, r in enumerate(self.rows) for d, j in r)
        idx = [-1] * self.k; used = set()
        for d, a, j in pairs:
            if idx[a] == -1 and j not in used:
                idx[a] = j; used.add(j)
        return idx, value(self.rows, idx, self.gate)

    def failures(self, idx, d2, na=None):
        """[(position, what)] of a frame's result (idx, d2, n_admissible in the frame's order) that the reference rejects"""
        from assoc_nn_ref import mpf
        bad = []; idx = [int(j) for j in idx]; used = {}
        for a, j in enumerate(idx):
            if na is not None and not self.n_sure[a] <= int(na[a]) <= self.n_poss[a]:
                bad.append((a, "n_admissible %d outside [%d, %d]" % (int(na[a]), self.n_sure[a], self.n_poss[a])))
            if j == -1:
                if d2[a] != INF:
                    bad.append((a, "-1 without +inf"))
                continue
            if j in used:
                bad.append((a, "cone %d taken twice (also by %d)" % (j, used[j])))
            used.setdefault(j, a)
            cd = self.pairs.get((a, j))
            if cd is None:
                bad.append((a, "cone %d is not possibly admissible" % j)); continue
            if not self.in_cut[(a, j)]:
                bad.append((a, "cone %d is surely not among the observation's 8 best" % j))
            r = abs(mpf(float(d2[a])) - cd.d2) / cd.B if cd.B > 0 else (0 if mpf(float(d2[a])) == cd.d2 else INF)
            if not r <= 1:
                bad.append((a, "d2 %.17g off the exact %.17g by %.3g B" % (d2[a], float(cd.d2), float(r))))
        for a, j in enumerate(idx):
            if j == -1:
                free = [c for (b, c), s in self.sure_in.items() if b == a and s and c not in used]
                if free:
                    bad.append((a, "-1 where cone %d, surely on the list, remains free" % free[0]))
        if self.decided:
            for a, j in enumerate(idx):
                if j != self.expect[a]:
                    bad.append((a, "index %d, the exact optimum has %d" % (j, self.expect[a])))
        return bad
