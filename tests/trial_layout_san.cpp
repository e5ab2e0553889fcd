// The carving of the step-control methods' device buffer (csrc/gs_trial.hpp) under the host sanitizers: a stand-alone program, no HIP.
// For Levenberg-Marquardt's and the dogleg's array lists at NP + ML = 0, 1, 255, 256, 257 and over a growth that crosses the
// capacity: every offset on a multiple of 256 bytes, no two arrays overlapping (each array is written through a host buffer of
// `total` bytes, so an overrun is the sanitizer's), the total equal to the last end, and every figure equal to the arithmetic
// gs_solve.cpp's lm_reserve / dl_reserve did by hand before the header existed, restated below as plain formulas.
#include "gs_trial.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

using namespace gs;

static int bad = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++bad; } } while (0)
static size_t al(size_t b) { return (b + 255) & ~(size_t)255; }
// the two methods' lists as gs_solve.cpp passes them (rec: bytes of one state record).  LM: hist_lambda, one partial array.  Dogleg:
// hist_delta, hist_kind, its partial arrays, and b, H b, h_dl, H h_dl
static TrialExtras lm_list(size_t rec) { return {2 * rec, 1, 0, 1, 0}; }
static TrialExtras dl_list(size_t rec, int part_arrays) { return {2 * rec, 1, 1, part_arrays, 4}; }
// the grow-only rule of trial_reserve: an allocation is kept while the graph fits its capacities
static bool trial_fits(size_t cap_p, size_t cap_l, size_t NP, size_t ML) { return !(NP > cap_p || ML > cap_l); }

// (offset, bytes) of every array of a layout, in address order as the formulas below list them
static std::vector<std::pair<size_t, size_t>> blocks(const TrialLayout &L, const TrialExtras &x) {
    std::vector<std::pair<size_t, size_t>> b;
    b.push_back({L.state, x.state_bytes}); b.push_back({L.hist_chi2, 64 * 8});
    for (int k = 0; k < x.hist_f64; ++k) b.push_back({L.hist_f64[k], 64 * 8});
    b.push_back({L.hist_trials, 64 * 4});
    for (int k = 0; k < x.hist_i32; ++k) b.push_back({L.hist_i32[k], 64 * 4});
    b.push_back({L.base_pose, L.cp * 24}); b.push_back({L.base_cs, L.cp * 16}); b.push_back({L.base_lm, L.cl * 16});
    b.push_back({L.part, (size_t)x.part_arrays * L.cpart * 8});
    for (int k = 0; k < x.vec_pairs; ++k) { b.push_back({L.vec_pose[k], L.cp * 24}); b.push_back({L.vec_lm[k], L.cl * 16}); }
    return b;
}
static void check_layout(const TrialLayout &L, const TrialExtras &x, size_t NP, size_t ML) {
    CHECK(L.cp == NP + 64 && L.cl == ML + 64 && L.cpart == (L.cp + L.cl + 255) / 256 + 1);
    CHECK(L.cpart >= (NP + ML + 255) / 256);                          // one partial per workgroup of the vertex-parallel grid
    auto b = blocks(L, x);
    std::vector<unsigned char> mem(L.total, 0);
    size_t end = 0;
    for (size_t i = 0; i < b.size(); ++i) {
        CHECK(b[i].first % 256 == 0);
        CHECK(b[i].first >= end);                                     // address order, no overlap with the one before
        for (size_t k = 0; k < b[i].second; ++k) CHECK(mem[b[i].first + k]++ == 0);      // nor with any other
        end = b[i].first + al(b[i].second);
    }
    CHECK(L.total == end);
}
// what lm_reserve computed: state, hist_chi2, hist_lambda, hist_trials, base_pose, base_cs, base_lm, part
static void check_lm(size_t NP, size_t ML, size_t rec) {
    const TrialExtras x = lm_list(rec); const TrialLayout L = trial_carve(NP, ML, x);
    check_layout(L, x, NP, ML);
    const size_t cp = NP + 64, cl = ML + 64, cpart = (cp + cl + 255) / 256 + 1;
    const size_t o_state = 0, o_hc = al(2 * rec), o_hl = o_hc + al(64 * 8), o_ht = o_hl + al(64 * 8), o_bp = o_ht + al(64 * 4),
                 o_bc = o_bp + al(cp * 24), o_bl = o_bc + al(cp * 16), o_part = o_bl + al(cl * 16), total = o_part + al(cpart * 8);
    CHECK(L.state == o_state && L.hist_chi2 == o_hc && L.hist_f64[0] == o_hl && L.hist_trials == o_ht && L.base_pose == o_bp);
    CHECK(L.base_cs == o_bc && L.base_lm == o_bl && L.part == o_part && L.total == total);
}
// what dl_reserve computed: state, hist_chi2, hist_delta, hist_trials, hist_kind, base_*, 9 partial arrays, then 4 pairs of vectors
static void check_dl(size_t NP, size_t ML, size_t rec) {
    const int n_part = 9;
    const TrialExtras x = dl_list(rec, n_part); const TrialLayout L = trial_carve(NP, ML, x);
    check_layout(L, x, NP, ML);
    const size_t cp = NP + 64, cl = ML + 64, cpart = (cp + cl + 255) / 256 + 1;
    size_t total = 0;
    auto take = [&total](size_t b) { const size_t o = total; total += (b + 255) & ~(size_t)255; return o; };
    const size_t o_state = take(2 * rec), o_hc = take(64 * 8), o_hd = take(64 * 8), o_ht = take(64 * 4), o_hk = take(64 * 4),
                 o_bp = take(cp * 24), o_bc = take(cp * 16), o_bl = take(cl * 16), o_part = take(n_part * cpart * 8);
    CHECK(L.state == o_state && L.hist_chi2 == o_hc && L.hist_f64[0] == o_hd && L.hist_trials == o_ht && L.hist_i32[0] == o_hk);
    CHECK(L.base_pose == o_bp && L.base_cs == o_bc && L.base_lm == o_bl && L.part == o_part);
    for (int k = 0; k < 4; ++k) { const size_t vp = take(cp * 24), vl = take(cl * 16); CHECK(L.vec_pose[k] == vp && L.vec_lm[k] == vl); }
    CHECK(L.total == total);
}

int main() {
    const size_t recs[] = {88, 96, 104, 128, 129};                    // record sizes around a 256-byte step of the doubled record
    const size_t sums[] = {0, 1, 255, 256, 257};
    for (size_t rec : recs) for (size_t n : sums) {
        const size_t splits[][2] = {{n, 0}, {0, n}, {n - n / 4, n / 4}};
        for (auto &s : splits) { check_lm(s[0], s[1], rec); check_dl(s[0], s[1], rec); }
    }
    // grow-only: the allocation made for (NP, ML) is kept up to its capacities and replaced by a larger one one vertex beyond
    const size_t NP = 200, ML = 56; const TrialLayout L = trial_carve(NP, ML, lm_list(104));
    CHECK(trial_fits(L.cp, L.cl, NP, ML) && trial_fits(L.cp, L.cl, L.cp, L.cl));
    CHECK(!trial_fits(L.cp, L.cl, L.cp + 1, ML) && !trial_fits(L.cp, L.cl, NP, L.cl + 1) && !trial_fits(0, 0, 0, 1));
    const TrialLayout G = trial_carve(L.cp + 1, ML, lm_list(104));
    CHECK(G.cp == L.cp + 65 && G.total > L.total && trial_fits(G.cp, G.cl, L.cp + 1, ML));
    check_lm(L.cp + 1, ML, 104); check_dl(NP, L.cl + 1, 88);
    std::printf(bad ? "trial layout: %d checks FAILED\n" : "trial layout: ok\n", bad);
    return bad ? 1 : 0;
}
