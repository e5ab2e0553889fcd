// edge_mask_san.cpp — stand-alone check of the host side of edge deactivation (csrc/gs_edge_mask_host.hpp: the flag store and its
// growth with the edge arrays, the scan for isolated vertices, the keep_connected rule, the "what does the device hold" bookkeeping),
// with its own main().  Built and run on the host with the sanitizers, no HIP and no GPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/edge_mask_san.cpp -o edge_mask_san && ./edge_mask_san
#include "../opendlv-logic-cfsd18-sensation-slam_amd/csrc/gs_edge_mask_host.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace gs;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

struct Graph {
    std::vector<uint8_t> pf, lf, pprior, lprior;
    std::vector<int32_t> pp_i, pp_j, pl_p, pl_l;
    MaskGraphView view() const {
        MaskGraphView v;
        v.N = (int32_t)pf.size(); v.M = (int32_t)lf.size(); v.Epp = (int32_t)pp_i.size(); v.Epl = (int32_t)pl_p.size();
        v.pose_fixed = pf.data(); v.lm_fixed = lf.data(); v.pp_i = pp_i.data(); v.pp_j = pp_j.data(); v.pl_p = pl_p.data(); v.pl_l = pl_l.data();
        v.pose_prior = pprior.data(); v.lm_prior = lprior.data();
        return v;
    }
};

static Graph random_graph(std::mt19937 &rng, int N, int M, int obs) {
    Graph g;
    g.pf.assign((size_t)N, 0); g.lf.assign((size_t)M, 0); g.pprior.assign((size_t)N, 0); g.lprior.assign((size_t)M, 0);
    g.pf[0] = 1; if (M > 3) g.lf[3] = 1;
    for (int k = 0; k < N; k += 11) g.pprior[(size_t)k] = 1;
    for (int k = 1; k < M; k += 6) g.lprior[(size_t)k] = 1;
    for (int p = 0; p + 1 < N; ++p) { g.pp_i.push_back(p); g.pp_j.push_back(p + 1); }
    for (int k = 0; k < 5; ++k) { g.pp_i.push_back((int32_t)(rng() % (unsigned)N)); g.pp_j.push_back((int32_t)(rng() % (unsigned)N)); }     // loop closures (a self-edge may occur)
    for (int p = 0; p < N; ++p) for (int k = 0; k < obs; ++k) { g.pl_p.push_back(p); g.pl_l.push_back((int32_t)(rng() % (unsigned)M)); }
    return g;
}

// the scan, restated: a vertex counts every active edge that touches it
static bool isolated_ref(const Graph &g, const EdgeMaskStore &s, int32_t &kind, int32_t &index) {
    for (int32_t p = 0; p < (int32_t)g.pf.size(); ++p) {
        if (g.pf[(size_t)p] || g.pprior[(size_t)p]) continue;
        bool any = false;
        for (size_t k = 0; k < g.pp_i.size(); ++k) any = any || (s.active(0, (int64_t)k) && (g.pp_i[k] == p || g.pp_j[k] == p));
        for (size_t k = 0; k < g.pl_p.size(); ++k) any = any || (s.active(1, (int64_t)k) && g.pl_p[k] == p);
        if (!any) { kind = 0; index = p; return true; } }
    for (int32_t l = 0; l < (int32_t)g.lf.size(); ++l) {
        if (g.lf[(size_t)l] || g.lprior[(size_t)l]) continue;
        bool any = false;
        for (size_t k = 0; k < g.pl_l.size(); ++k) any = any || (s.active(1, (int64_t)k) && g.pl_l[k] == l);
        if (!any) { kind = 1; index = l; return true; } }
    return false;
}

static void store_case() {
    EdgeMaskStore S;
    CHECK(S.empty() && !S.any_off() && S.active(0, 0) && S.active(1, 1000000) && S.active(0, -1));
    const uint64_t v0 = S.version;
    CHECK(!S.set(0, 5, 10, true) && S.empty() && S.version == v0);              // activating an active edge allocates nothing
    CHECK(!S.set(0, 10, 10, false) && !S.set(0, -1, 10, false) && S.empty());    // out of range
    CHECK(S.set(0, 5, 10, false) && S.act[0].size() == 10 && S.n_off[0] == 1 && !S.active(0, 5) && S.active(0, 4) && S.version == v0 + 1);
    CHECK(!S.set(0, 5, 10, false) && S.version == v0 + 1);
    CHECK(S.active(0, 17));                                                     // an edge added later: active, beyond the vector
    CHECK(!S.set(0, 17, 20, true) && S.act[0].size() == 10);
    CHECK(S.set(0, 17, 20, false) && S.act[0].size() == 20 && S.n_off[0] == 2 && !S.active(0, 5) && S.active(0, 12));   // growth keeps the old flags
    CHECK(S.set(1, 0, 3, false) && S.n_off[1] == 1 && S.any_off());
    CHECK(S.set(0, 5, 20, true) && S.n_off[0] == 1);
    CHECK(S.activate_all() && !S.any_off() && !S.empty() && S.active(0, 17) && S.active(1, 0));
    CHECK(!S.activate_all());
    S.clear();
    CHECK(S.empty() && !S.any_off());
}

static void sync_case() {
    EdgeMaskStore S; EdgeMaskSync Y;
    int32_t n[2] = {8, 6};
    std::vector<int32_t> ch[2];
    CHECK(Y.needed(S.version, 0, 0, 0));
    S.set(0, 2, n[0], false); S.set(1, 5, n[1], false);
    Y.changes(S, n, 1, ch); CHECK(ch[0].size() == 1 && ch[0][0] == 2 && ch[1].size() == 1 && ch[1][0] == 5);
    Y.changes(S, n, 1, ch); CHECK(ch[0].size() == 1 && ch[1].size() == 1);       // not committed: listed again
    Y.commit(S, n, ch); Y.done(S.version, 1, 7, 0);
    CHECK(!Y.needed(S.version, 1, 7, 0) && Y.needed(S.version, 2, 7, 0) && Y.needed(S.version, 1, 8, 0) && Y.needed(S.version, 1, 7, 1));
    Y.changes(S, n, 1, ch); CHECK(ch[0].empty() && ch[1].empty());
    S.set(0, 2, n[0], true); S.set(0, 3, n[0], false);
    Y.changes(S, n, 1, ch); CHECK(ch[0].size() == 2 && ch[0][0] == 2 && ch[0][1] == 3 && ch[1].empty());
    Y.commit(S, n, ch);
    n[0] = 12;                                                                   // growth: four more odometry edges, one switched off at once
    S.set(0, 11, n[0], false);
    Y.changes(S, n, 1, ch); CHECK(ch[0].size() == 1 && ch[0][0] == 11);
    Y.commit(S, n, ch); CHECK(Y.have[0].size() == 12 && Y.have[0][11] == 0 && Y.have[0][10] == 1 && Y.have[0][3] == 0);
    Y.changes(S, n, 2, ch);                                                      // a full upload: every inactive edge again, nothing else
    CHECK(ch[0].size() == 2 && ch[0][0] == 3 && ch[0][1] == 11 && ch[1].size() == 1 && ch[1][0] == 5);
    Y.commit(S, n, ch);
    S.activate_all();
    Y.changes(S, n, 2, ch); CHECK(ch[0].size() == 2 && ch[1].size() == 1);
    Y.invalidate(); CHECK(Y.have[0].empty() && Y.needed(S.version, 2, 7, 0));
}

static void random_case(unsigned seed, int N, int M, int obs) {
    std::mt19937 rng(seed);
    Graph g = random_graph(rng, N, M, obs);
    const MaskGraphView v = g.view();
    EdgeMaskStore S;
    int32_t kind = -1, index = -1, rk = -1, ri = -1;
    for (int round = 0; round < 6; ++round) {
        // random flags, then the scan against its restatement
        for (int t = 0; t < (v.Epp + v.Epl) / 3; ++t) {
            const int kd = (int)(rng() & 1u); const int32_t n = kd == 0 ? v.Epp : v.Epl;
            S.set(kd, (int32_t)(rng() % (unsigned)n), n, (rng() % 3u) == 0); }
        int32_t off[2] = {0, 0};
        for (int kd = 0; kd < 2; ++kd) for (int32_t k = 0; k < (kd == 0 ? v.Epp : v.Epl); ++k) off[kd] += !S.active(kd, k);
        CHECK(off[0] == S.n_off[0] && off[1] == S.n_off[1]);
        const bool a = find_isolated(v, S, kind, index), b = isolated_ref(g, S, rk, ri);
        CHECK(a == b && (!a || (kind == rk && index == ri)));
        // keep_connected from a connected start never isolates a vertex
        S.activate_all();
        if (find_isolated(v, S, kind, index)) continue;                          // (a landmark nobody observes)
        for (int kd = 0; kd < 2; ++kd) {
            const int32_t n = kd == 0 ? v.Epp : v.Epl;
            std::vector<uint8_t> cand((size_t)n, 0);
            for (auto &c : cand) c = (rng() % 10u) < 7u;
            EdgeMaskStore T = S;
            const std::vector<int32_t> kept = deactivate_candidates(v, S, kd, cand.data(), true);
            CHECK(!find_isolated(v, S, kind, index));
            for (size_t t = 0; t < kept.size(); ++t) CHECK(cand[(size_t)kept[t]] && !S.active(kd, kept[t]) && (t == 0 || kept[t - 1] < kept[t]));
            CHECK((int32_t)kept.size() == S.n_off[kd] - T.n_off[kd]);
            // every skipped candidate would isolate an endpoint now
            for (int32_t k = 0; k < n; ++k) if (cand[(size_t)k] && S.active(kd, k)) {
                EdgeMaskStore U = S; U.set(kd, k, n, false);
                CHECK(find_isolated(v, U, kind, index)); }
            // without the rule every active candidate goes
            const std::vector<int32_t> all = deactivate_candidates(v, T, kd, cand.data(), false);
            int32_t want = 0; for (auto c : cand) want += c != 0;
            CHECK((int32_t)all.size() == want);                                  // (every edge of the kind was active in T)
            for (int32_t k = 0; k < n; ++k) CHECK(T.active(kd, k) == !cand[(size_t)k]);
        }
    }
}

int main() {
    store_case();
    sync_case();
    for (unsigned seed = 1; seed <= 12; ++seed) random_case(seed, 30 + (int)seed * 3, 12 + (int)seed, 2 + (int)(seed % 3));
    std::printf("edge mask host: ok\n");
    return 0;
}
