// dup_layout_san.cpp — a stand-alone program (its own main, no HIP) around csrc/gs_dup_host.hpp, built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_dup_cpu.py.  It carves a twins call's pieces out of a heap block of exactly DupLayout::bytes for
// every map size at an edge (the tile, the scan's thread, the limit) and writes every piece to its last byte, as the kernels and the copies do:
// a piece that overlaps its neighbour, leaves the block or breaks its alignment is found here.  Then it runs merge_landmarks on a small
// HostGraph with the landmark index lists of its priors and polar edges — keep before drop, keep behind drop, the last landmark — and
// compares every array and both lists with what the same insertions without `drop` give.
#include "gs_dup_host.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace gs;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

struct Piece { size_t off, bytes, align; unsigned char tag; };

static void layout(long long n) {
    DupLayout L;
    CHECK(dup_layout(n, L));
    std::vector<unsigned char> mem(L.bytes, 0);
    const size_t m = (size_t)n, nb = (size_t)dup_blocks(n);
    CHECK(nb * DUP_BLOCK >= m && (nb == 0 || (nb - 1) * DUP_BLOCK < m) && nb <= (size_t)DUP_BLOCKS_MAX);
    const std::vector<Piece> ps = {{L.in_xy, m * 16, 16, 1}, {L.in_type, m * 4, 4, 2}, {L.in_cov, m * 32, 32, 3}, {L.twin, m * 4, 4, 4}, {L.d2, m * 8, 8, 5},
                                   {L.second, m * 8, 8, 6}, {L.nadm, m * 4, 4, 7}, {L.slot, m * 4, 4, 8}, {L.f_xy, m * 16, 16, 9}, {L.f_cov, m * 32, 32, 10},
                                   {L.blk, 3 * nb * 4, 4, 11}, {L.blk_off, nb * 4, 4, 12}, {L.info, 16, 4, 13}, {L.out_xy, m * 16, 16, 14},
                                   {L.out_type, m * 4, 4, 15}, {L.out_cov, m * 32, 32, 16}, {L.remap, m * 4, 4, 17}};
    for (const Piece &p : ps) { CHECK(p.off % 256 == 0 && p.off % p.align == 0); CHECK(p.off + p.bytes <= mem.size());
        if (p.bytes && p.off + p.bytes <= mem.size()) std::memset(mem.data() + p.off, p.tag, p.bytes); }
    for (const Piece &p : ps)                                                  // nobody wrote into anybody else
        for (size_t b = 0; b < p.bytes && p.off + b < mem.size(); ++b) if (mem[p.off + b] != p.tag) { CHECK(!"a piece was overwritten"); break; }
}

// a graph of 3 poses and `ids` landmarks; landmark `skip` (an id, or -1) is left out and its edges and priors point at `to`
static void build(HostGraph &h, std::vector<int32_t> &prior_v, std::vector<int32_t> &polar_v, const std::vector<int32_t> &ids, int32_t skip, int32_t to) {
    for (int p = 0; p < 3; ++p) { h.pose_index[10 + p] = h.n_poses(); h.pose_id.push_back(10 + p); h.pose_fixed.push_back(p == 0);
        for (int c = 0; c < 3; ++c) h.pose_est.push_back(p + 0.25 * c); }
    for (int32_t id : ids) { if (id == skip) continue;
        h.lm_index[id] = h.n_lms(); h.lm_id.push_back(id); h.lm_fixed.push_back(id == 100); h.lm_est.push_back(id * 0.5); h.lm_est.push_back(id * -0.25); }
    int e = 0;
    for (int p = 0; p < 3; ++p) for (int32_t id : ids) { if ((e++ % 3) == 2) continue;          // two of three (pose, landmark) pairs carry an edge
        const int32_t at = id == skip ? to : id;
        h.pl_p.push_back(p); h.pl_l.push_back(h.lm_index[at]); h.pl_z.push_back(p + id); h.pl_z.push_back(p - id);
        h.pl_info.push_back(1.0 + e); h.pl_info.push_back(0.0); h.pl_info.push_back(2.0 + e);
        if (e % 2 == 0) polar_v.push_back(h.lm_index[at]); }                        // every other edge is a polar one: PolarStore::lm_v's entry
    for (int32_t id : ids) if (id % 2 == 0) prior_v.push_back(h.lm_index[id == skip ? to : id]);
}

static void merge(const std::vector<int32_t> &ids, int32_t keep, int32_t drop) {
    HostGraph a, b; std::vector<int32_t> pa, pb, qa, qb;
    build(a, pa, qa, ids, -1, -1); build(b, pb, qb, ids, drop, keep);
    const uint64_t sv = a.structure_version, rv = a.reshape_version;
    CHECK(!qa.empty() && merge_landmarks(a, pa, qa, a.lm_index[keep], a.lm_index[drop]));
    CHECK(a.structure_version == sv + 1 && a.reshape_version == rv + 1);
    CHECK(a.lm_id == b.lm_id && a.lm_est == b.lm_est && a.lm_fixed == b.lm_fixed && a.lm_index == b.lm_index);
    CHECK(a.pl_p == b.pl_p && a.pl_l == b.pl_l && a.pl_z == b.pl_z && a.pl_info == b.pl_info && pa == pb && qa == qb);
    CHECK(a.pose_id == b.pose_id && a.pose_est == b.pose_est && a.pose_fixed == b.pose_fixed);
    for (int32_t l : a.pl_l) CHECK(l >= 0 && l < a.n_lms());
    for (int32_t l : pa) CHECK(l >= 0 && l < a.n_lms());
    for (int32_t l : qa) CHECK(l >= 0 && l < a.n_lms());
}

int main() {
    DupLayout L;
    CHECK(!dup_layout(-1, L) && !dup_layout((long long)DUP_MAP_MAX + 1, L));
    const long long sizes[] = {0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 65536, DUP_MAP_MAX - 1, DUP_MAP_MAX};
    for (long long n : sizes) layout(n);
    const std::vector<int32_t> ids = {100, 7, 42, 3, 18};
    merge(ids, 100, 42); merge(ids, 42, 7); merge(ids, 7, 18); merge(ids, 18, 3); merge(ids, 3, 18); merge({5, 6}, 5, 6); merge({5, 6}, 6, 5);
    { HostGraph h; std::vector<int32_t> pv, qv; build(h, pv, qv, ids, -1, -1); const HostGraph before = h; const std::vector<int32_t> qv0 = qv;
      CHECK(!merge_landmarks(h, pv, qv, 1, 1) && !merge_landmarks(h, pv, qv, -1, 2) && !merge_landmarks(h, pv, qv, 0, 5));
      CHECK(h.lm_id == before.lm_id && h.pl_l == before.pl_l && qv == qv0 && h.structure_version == before.structure_version); }
    if (fails == 0) std::printf("dup layout: ok\n");
    return fails ? 1 : 0;
}
