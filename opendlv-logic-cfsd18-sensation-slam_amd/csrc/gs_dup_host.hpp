// gs_dup_host.hpp — the host side of the map twins (host arithmetic only, no HIP: tests/dup_layout_san.cpp compiles it alone).
//   DupLayout         a twins call's device memory for a map of n cones, as byte offsets into one allocation; every piece starts on a
//                     256-byte boundary (xy needs 16, cov 32)
//   merge_landmarks   g2o's mergeVertices(keep, drop, erase = true) on HostGraph and the landmark index lists of the priors and the polar edges
#pragma once
#include "gs_host.hpp"

#include <cstddef>
#include <cstdint>
#include <vector>

namespace gs {

static constexpr int DUP_MAP_MAX = 262144;                                     // GS_DUP_MAP_MAX
static constexpr int DUP_BLOCK = 256;                                          // cones a workgroup: the search's tile and the scan's block
static constexpr int DUP_BLOCKS_MAX = DUP_MAP_MAX / DUP_BLOCK;                 // what the one-workgroup scan takes: four blocks a thread

inline size_t dup_pad(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
inline int dup_blocks(long long n) { return (int)((n + DUP_BLOCK - 1) / DUP_BLOCK); }

struct DupLayout {
    size_t in_xy, in_type, in_cov;                       // a batch call's upload of the map (a resident call reads the handle's arrays)
    size_t twin, d2, second, nadm;                       // the search's outputs, [n] each
    size_t slot;                                         // [n] a kept cone's rank among the kept of its block, -1 for a dropped one
    size_t f_xy, f_cov;                                  // [n][2], [n][4] what a kept cone carries into the consolidated map
    size_t blk;                                          // [3][blocks] kept cones, twin pairs, ambiguous cones of each block
    size_t blk_off;                                      // [blocks] the kept cones of the blocks below
    size_t info;                                         // gs_dup_info
    size_t out_xy, out_type, out_cov, remap;             // the consolidated map (the second buffer) and the index table
    size_t bytes;
};
// false (and nothing set) outside 0 <= n <= DUP_MAP_MAX
inline bool dup_layout(long long n, DupLayout &L) {
    if (n < 0 || n > DUP_MAP_MAX) return false;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += dup_pad(bytes ? bytes : 1); return at; };
    const size_t m = (size_t)n, nb = (size_t)dup_blocks(n);
    L.in_xy = take(m * 16); L.in_type = take(m * 4); L.in_cov = take(m * 32);
    L.twin = take(m * 4); L.d2 = take(m * 8); L.second = take(m * 8); L.nadm = take(m * 4);
    L.slot = take(m * 4); L.f_xy = take(m * 16); L.f_cov = take(m * 32);
    L.blk = take(3 * nb * 4); L.blk_off = take(nb * 4); L.info = take(16);
    L.out_xy = take(m * 16); L.out_type = take(m * 4); L.out_cov = take(m * 32); L.remap = take(m * 4);
    L.bytes = off;
    return true;
}

// Landmark `drop` (an index) merged into landmark `keep`: its observation edges, its priors (prior_lm_v: the landmark priors' vertex
// indices, insertion order) and its polar edges (polar_lm_v: the polar edges' landmark indices, insertion order — PolarStore keeps one
// beside the carrier's observation index) point at keep, it is erased, the landmarks behind it move down by one in all three lists, lm_index
// is rebuilt, and the structure and reshape versions move so that the next plan is a full one.  Edges and priors keep their places, so
// whatever is stored by edge index (activity flags, polar measurements) stays with its edge.  The caller bumps the two stores' versions.
// False (nothing changed): an index out of range, or keep == drop.
inline bool merge_landmarks(HostGraph &h, std::vector<int32_t> &prior_lm_v, std::vector<int32_t> &polar_lm_v, int keep, int drop) {
    const int M = h.n_lms();
    if (keep < 0 || drop < 0 || keep >= M || drop >= M || keep == drop) return false;
    auto moved = [&](int32_t l) { return l == drop ? (keep > drop ? keep - 1 : keep) : l > drop ? l - 1 : l; };
    for (int32_t &l : h.pl_l) l = moved(l);
    for (int32_t &l : prior_lm_v) l = moved(l);
    for (int32_t &l : polar_lm_v) l = moved(l);
    h.lm_id.erase(h.lm_id.begin() + drop);
    h.lm_est.erase(h.lm_est.begin() + 2 * (size_t)drop, h.lm_est.begin() + 2 * (size_t)drop + 2);
    h.lm_fixed.erase(h.lm_fixed.begin() + drop);
    h.lm_index.clear();
    for (int l = 0; l < M - 1; ++l) h.lm_index[h.lm_id[(size_t)l]] = l;
    ++h.structure_version; ++h.reshape_version;
    return true;
}

}  // namespace gs
