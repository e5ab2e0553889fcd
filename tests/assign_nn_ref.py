"""The one-to-one association inside a frame (TEST-ONLY), written from include/graphslam.h ("one-to-one association") — not from the kernel:
the greedy matching over a frame's admissible pairs in ascending (d2, observation index, cone index), twice over (the sorted walk and the
"mutual best" rounds the header states as its consequence), the proposer-only shortcut that is NOT the rule, and the checker that holds a
device result to the exact reference of assoc_nn_ref.py.

A distance matrix D is [k observations, m cones] with +inf (or None in an object matrix) where the pair is not admissible; the columns are in
ascending cone index, `cones` names them.  Entries may be floats or mpmath numbers: only comparisons are made.

DECIDED.  The exact reference knows every pair's d2 to within its bound B and whether it is surely / possibly admissible.  A frame is DECIDED
when every candidate pair of the frame is surely admissible or surely not (poss == sure) and any two possibly-admissible pairs that share an
observation or a cone have disjoint intervals [d2 - B, d2 + B]: then no rounding of the device can change an order the greedy walk depends on
(it only ever chooses between pairs that share an observation or a cone), and the device's indices must equal the greedy on the exact d2.
Whatever the frame, a result must be a valid matching (no cone twice, every taken pair possibly admissible, d2 within the pair's B), and an
observation left at -1 must have no surely-admissible cone that the frame left free (the greedy matching is maximal)."""
import numpy as np

INF = float("inf")


def _open(v):
    return v is not None and v != INF


def greedy(D, cones=None):
    """(index [k], d2 [k]) of the sorted walk; index holds cone names (column numbers when cones is None), -1 / +inf where none"""
    k = len(D); m = len(D[0]) if k else 0
    cones = list(range(m)) if cones is None else list(cones)
    pairs = sorted((D[i][c], i, cones[c]) for i in range(k) for c in range(m) if _open(D[i][c]))
    idx = [-1] * k; d2 = [INF] * k; used = set()
    for d, i, j in pairs:
        if idx[i] == -1 and j not in used:
            idx[i] = j; d2[i] = d; used.add(j)
    return idx, d2


def mutual_best(D, cones=None, proposers_only=False):
    """(index, d2, rounds) of the rounds of the header: every unassigned observation proposes its best unclaimed cone by (d2, j); (i, c) commits
    iff no other unassigned observation i' has an admissible d2(i', c) with (d2, i') below (d2(i, c), i).  proposers_only=True is the SHORTCUT
    that asks only the observations that proposed c — a different matching, kept to show that the tests tell the two apart"""
    k = len(D); m = len(D[0]) if k else 0
    cones = list(range(m)) if cones is None else list(cones)
    idx = [-1] * k; d2 = [INF] * k; claimed = set(); final = set(); rounds = 0
    while True:
        prop = {}
        for i in range(k):
            if idx[i] != -1 or i in final:
                continue
            best = min(((D[i][c], c) for c in range(m) if _open(D[i][c]) and c not in claimed), default=None)
            if best is None:
                final.add(i)
            else:
                prop[i] = best
        if not prop:
            return idx, d2, rounds
        rounds += 1
        commit = []
        for i, (d, c) in prop.items():
            rivals = [o for o in prop if prop[o][1] == c] if proposers_only else list(prop)
            if not any(o != i and _open(D[o][c]) and (D[o][c], o) < (d, i) for o in rivals):
                commit.append((i, d, c))
        assert commit, "a round always commits the smallest open pair"
        for i, d, c in commit:
            idx[i] = cones[c]; d2[i] = d; claimed.add(c)


def frames_by_pose(pose_of):
    """(order, frame_start): the observations grouped by pose in stable order — frame f is order[frame_start[f] : frame_start[f + 1]]"""
    pose_of = np.asarray(pose_of); order = np.argsort(pose_of, kind="stable")
    _, counts = np.unique(pose_of, return_counts=True)
    return order, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def has_duplicates(idx):
    a = np.asarray(idx); a = a[a >= 0]
    return len(np.unique(a)) != len(a)


class FrameRef:
    """one frame against the exact reference R (assoc_nn_ref.Ref): members = the reference's observation numbers in the frame's order"""

    def __init__(self, R, members):
        self.R = R; self.members = [int(i) for i in members]
        self.pairs = {}                                                       # (position in the frame, cone) -> Cand, possibly admissible only
        undecided = False
        for a, i in enumerate(self.members):
            for cd in R.cands[i]:
                if cd.poss != cd.sure:
                    undecided = True
                if cd.poss:
                    self.pairs[(a, cd.j)] = cd
        keys = list(self.pairs)
        by_obs, by_cone = {}, {}
        for (a, j) in keys:
            by_obs.setdefault(a, []).append((a, j)); by_cone.setdefault(j, []).append((a, j))
        for group in list(by_obs.values()) + list(by_cone.values()):
            iv = sorted((self.pairs[p].d2 - self.pairs[p].B, self.pairs[p].d2 + self.pairs[p].B) for p in group)
            if any(iv[t + 1][0] <= iv[t][1] for t in range(len(iv) - 1)):
                undecided = True
        self.decided = not undecided
        self.cones = sorted({j for (_, j) in keys})
        col = {j: c for c, j in enumerate(self.cones)}
        D = [[None] * len(self.cones) for _ in self.members]
        for (a, j), cd in self.pairs.items():
            D[a][col[j]] = cd.d2
        self.D = D
        self.expect = greedy(D, self.cones)[0] if self.cones else [-1] * len(self.members)
        best = [min(((D[a][c], self.cones[c]) for c in range(len(self.cones)) if D[a][c] is not None), default=(None, -1))[1] for a in range(len(self.members))]
        taken = [j for j in best if j >= 0]
        self.contested = len(set(taken)) != len(taken)                       # a cone is the best match of two observations

    def failures(self, idx, d2):
        """[(position, what)] of a frame's result (idx, d2 in the frame's order) that the reference rejects"""
        from assoc_nn_ref import mpf
        bad = []; idx = [int(j) for j in idx]; used = {}
        for a, j in enumerate(idx):
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
            r = abs(mpf(float(d2[a])) - cd.d2) / cd.B if cd.B > 0 else (0 if mpf(float(d2[a])) == cd.d2 else INF)
            if not r <= 1:
                bad.append((a, "d2 %.17g off the exact %.17g by %.3g B" % (d2[a], float(cd.d2), float(r))))
        for a, j in enumerate(idx):
            if j == -1:
                free = [c for (b, c), cd in self.pairs.items() if b == a and cd.sure and c not in used]
                if free:
                    bad.append((a, "-1 where the surely admissible cone %d remains free" % free[0]))
        if self.decided:
            for a, j in enumerate(idx):
                if j != self.expect[a]:
                    bad.append((a, "index %d, the greedy on the exact d2 gives %d" % (j, self.expect[a])))
        return bad
