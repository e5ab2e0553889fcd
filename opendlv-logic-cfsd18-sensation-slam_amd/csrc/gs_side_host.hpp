// gs_side_host.hpp — what the host sides of the three side passes (gs_prior_host.hpp, gs_edge_mask_host.hpp, gs_polar_host.hpp) share:
// the angle normalisation, the grouping of records by vertex, the "does the device copy need to go up again" stamp and the layout of
// a device arena.  No HIP in here: the tests/*_san.cpp programs compile it with the host sanitizers.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace gs {

inline double normalize_theta(double th) {           // g2o normalize_theta: into [-pi, pi)
    if (th >= -M_PI && th < M_PI) return th;
    const double m = std::floor(th / (2 * M_PI)); th -= m * 2 * M_PI;
    if (th >= M_PI) th -= 2 * M_PI;
    if (th < -M_PI) th += 2 * M_PI;
    return th;
}

// Stable counting sort of items by key (values in [0, n_key)); skip[k] != 0 leaves item k out (nullptr: none).  ids = the keys that
// occur (ascending), start = the run starts ([ids.size() + 1]), order = the items sorted by key, insertion order inside a run
inline void group_by_key(const std::vector<int32_t> &key, int n_key, const uint8_t *skip, std::vector<int32_t> &ids, std::vector<int32_t> &start,
                         std::vector<int32_t> &order) {
    ids.clear(); start.clear(); order.clear();
    std::vector<int32_t> slot((size_t)n_key + 1, 0);              // counts, then key -> next free place of its run
    for (size_t k = 0; k < key.size(); ++k) if (!skip || !skip[k]) ++slot[(size_t)key[k]];
    int32_t at = 0;
    for (int v = 0; v < n_key; ++v) if (slot[(size_t)v] > 0) { const int32_t c = slot[(size_t)v]; ids.push_back(v); start.push_back(at); slot[(size_t)v] = at; at += c; }
    start.push_back(at);
    order.resize((size_t)at);
    for (size_t k = 0; k < key.size(); ++k) if (!skip || !skip[k]) order[(size_t)slot[(size_t)key[k]]++] = (int32_t)k;
}

// What the device holds against what the handle holds, over K version counters: the copy goes up again when it never did, was
// invalidated, or any counter moved
template <int K> struct SyncStamp {
    uint64_t at[K]; bool valid = false;
    SyncStamp() { for (uint64_t &v : at) v = ~0ull; }
    template <class... V> bool needed(V... now) const {
        static_assert(sizeof...(V) == K, "one value per counter");
        const uint64_t n[K] = {(uint64_t)now...};
        for (int k = 0; k < K; ++k) if (at[k] != n[k]) return true;
        return !valid;
    }
    template <class... V> void done(V... now) {
        static_assert(sizeof...(V) == K, "one value per counter");
        const uint64_t n[K] = {(uint64_t)now...};
        for (int k = 0; k < K; ++k) at[k] = n[k];
        valid = true;
    }
    void invalidate() { valid = false; }
};

// The blocks of one device allocation, one behind the other, each at a 256-byte-aligned offset (a block of zero bytes is legal: it
// takes no room and shares its offset with the next one)
struct ArenaLayout {
    size_t total = 0;
    size_t add(size_t bytes) { const size_t off = total; total += (bytes + 255) & ~(size_t)255; return off; }
};

}  // namespace gs
