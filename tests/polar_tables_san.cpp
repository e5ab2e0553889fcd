// polar_tables_san.cpp — stand-alone check of the host side of the polar observation edges (csrc/gs_polar_host.hpp: the store, the two
// groupings of one record set, the structure-of-arrays packing, locations in the main layout and in the tail, inactive flags, the
// refusals and the "does the device copy need to go up again" rule), with its own main().
// Built and run on the host with the sanitizers, no HIP and no GPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/polar_tables_san.cpp -o polar_tables_san && ./polar_tables_san
#include "../opendlv-logic-cfsd18-sensation-slam_amd/csrc/gs_polar_host.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace gs;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

// n_polar polar edges among Epl observation edges; edges >= base_Epl live in the tail; every `off_every`-th polar edge is inactive;
// hub >= 0: that pose carries every second polar edge (a pose with many edges)
static void random_case(unsigned seed, int N, int M, int Epl, int base_Epl, int n_polar, int off_every, int hub) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> u(0.5, 3.0);
    std::vector<int32_t> src((size_t)Epl);
    for (int k = 0; k < Epl; ++k) src[(size_t)k] = k < base_Epl ? 3 * k + 1 : -(k - base_Epl) - 1;
    std::vector<uint8_t> act((size_t)Epl, 1);
    PolarStore S;
    const uint64_t v0 = S.version;
    std::vector<int32_t> taken;
    for (int k = 0; k < n_polar; ++k) {
        const int32_t obs = (int32_t)((int64_t)k * Epl / n_polar);       // ascending, distinct (n_polar <= Epl)
        const int32_t p = hub >= 0 && k % 2 == 0 ? hub : (int32_t)(rng() % (unsigned)N), l = (int32_t)(rng() % (unsigned)M);
        const int32_t model = k % 3 == 0 ? 2 : 1;
        const double w[3] = {model == 2 ? 0.0 : u(rng), model == 2 ? 0.0 : 0.1 * u(rng), u(rng)};
        S.add(obs, model, p, l, model == 2 ? 0.0 : u(rng), 10.0 * u(rng) - 15.0, w);
        if (off_every > 0 && k % off_every == 0) act[(size_t)obs] = 0;
        taken.push_back(obs); }
    CHECK(S.version == v0 + (uint64_t)n_polar && S.n() == n_polar);
    for (int k = 0; k < n_polar; ++k) { const double zb = S.rec[(size_t)k * POLAR_REC + 1]; CHECK(zb >= -M_PI && zb < M_PI); }   // normalised when stored
    PolarTables T; std::string err;
    CHECK(build_polar_tables(S, N, M, Epl, src.data(), off_every > 0 ? act.data() : nullptr, T, err));
    const size_t n = (size_t)n_polar;
    CHECK(T.n_rec == n_polar && T.rec_pose.size() == n && T.rec_lm.size() == n && T.rec_src.size() == n && T.rec_obs.size() == n && T.lm_order.size() == n);
    CHECK(T.planes.size() == n * POLAR_REC && T.pv_start.size() == T.pv_id.size() + 1 && T.lv_start.size() == T.lv_id.size() + 1);
    CHECK(T.pv_start.front() == 0 && T.pv_start.back() == n_polar && T.lv_start.front() == 0 && T.lv_start.back() == n_polar);
    // pose side: every run holds exactly its pose's edges, insertion order inside the run; the record's fields are the store's
    std::vector<int> seen(n, 0);
    for (size_t j = 0; j < T.pv_id.size(); ++j) {
        CHECK(T.pv_start[j] < T.pv_start[j + 1] && (j == 0 || T.pv_id[j - 1] < T.pv_id[j]));
        int32_t r = T.pv_start[j];
        for (int k = 0; k < n_polar; ++k) if (S.pose_v[(size_t)k] == T.pv_id[j]) {
            CHECK(r < T.pv_start[j + 1]);
            CHECK(T.rec_pose[(size_t)r] == S.pose_v[(size_t)k] && T.rec_lm[(size_t)r] == S.lm_v[(size_t)k] && T.rec_obs[(size_t)r] == S.obs[(size_t)k]);
            CHECK(T.rec_src[(size_t)r] == src[(size_t)S.obs[(size_t)k]]);
            const bool on = off_every <= 0 || act[(size_t)S.obs[(size_t)k]] != 0;
            for (int c = 0; c < POLAR_REC; ++c) { const double want = (c >= 2 && !on) ? 0.0 : S.rec[(size_t)k * POLAR_REC + (size_t)c];
                CHECK(T.planes[(size_t)c * n + (size_t)r] == want); }
            ++seen[(size_t)r]; ++r; }
        CHECK(r == T.pv_start[j + 1]); }
    for (size_t r = 0; r < n; ++r) CHECK(seen[r] == 1);
    // landmark side: the same records, each once, grouped by landmark, in record order inside the run
    std::vector<int> seen_l(n, 0);
    for (size_t j = 0; j < T.lv_id.size(); ++j) {
        CHECK(T.lv_start[j] < T.lv_start[j + 1] && (j == 0 || T.lv_id[j - 1] < T.lv_id[j]));
        for (int32_t t = T.lv_start[j]; t < T.lv_start[j + 1]; ++t) { const int32_t r = T.lm_order[(size_t)t];
            CHECK(r >= 0 && r < n_polar && T.rec_lm[(size_t)r] == T.lv_id[j] && (t == T.lv_start[j] || T.lm_order[(size_t)t - 1] < r));
            ++seen_l[(size_t)r]; } }
    for (size_t r = 0; r < n; ++r) CHECK(seen_l[r] == 1);
    if (hub >= 0 && n_polar > 0) { size_t j = 0; while (j < T.pv_id.size() && T.pv_id[j] != hub) ++j;
        CHECK(j < T.pv_id.size() && T.pv_start[j + 1] - T.pv_start[j] >= (n_polar + 1) / 2); }
    if (base_Epl < Epl && n_polar > 0) { bool tail = false, main_ = false; for (int32_t s : T.rec_src) { tail = tail || s < 0; main_ = main_ || s >= 0; }
        CHECK(tail && main_); for (size_t r = 0; r < n; ++r) if (T.rec_src[r] < 0) CHECK(-(T.rec_src[r] + 1) == T.rec_obs[r] - base_Epl); }
}

int main() {
    {   // empty store
        PolarStore S; PolarTables T; std::string err;
        CHECK(S.empty() && S.n() == 0);
        const uint64_t v = S.version; S.clear(); CHECK(S.version == v);                 // clearing nothing is no change
        CHECK(build_polar_tables(S, 5, 4, 0, nullptr, nullptr, T, err));
        CHECK(T.n_rec == 0 && T.pv_id.empty() && T.lv_id.empty() && T.pv_start.size() == 1 && T.lv_start.size() == 1 && T.planes.empty());
        CHECK(build_polar_tables(S, 0, 0, 0, nullptr, nullptr, T, err) && T.n_rec == 0);
    }
    random_case(1, 40, 25, 160, 160, 60, 0, -1);
    random_case(2, 40, 25, 160, 160, 160, 0, -1);                                       // every observation edge polar
    random_case(3, 1000, 200, 6000, 6000, 2800, 5, -1);                                 // inactive flags
    random_case(4, 300, 80, 900, 900, 500, 0, 17);                                      // a pose with many edges
    random_case(5, 606, 130, 3000, 2960, 1400, 7, 603);                                 // tail locations, inactive flags, a tail pose with many edges
    random_case(6, 1, 1, 3, 2, 3, 1, 0);                                                // one pose, one cone, everything inactive
    {   // refusals: a vertex or a carrier that is not in the graph
        PolarStore S; const double w[3] = {1, 0, 1}; PolarTables T; std::string err; const int32_t src[4] = {0, 1, 2, 3};
        S.add(2, 1, 3, 1, 1.0, 0.5, w);
        CHECK(build_polar_tables(S, 4, 2, 4, src, nullptr, T, err));
        CHECK(!build_polar_tables(S, 3, 2, 4, src, nullptr, T, err) && !err.empty());   // pose 3 of 3
        CHECK(!build_polar_tables(S, 4, 1, 4, src, nullptr, T, err));                   // landmark 1 of 1
        CHECK(!build_polar_tables(S, 4, 2, 2, src, nullptr, T, err));                   // observation edge 2 of 2
        S.clear(); CHECK(S.empty());
    }
    {   // z_beta is normalised when stored, at and around the branch cut
        PolarStore S; const double w[3] = {1, 0, 1};
        const double in[6] = {M_PI, -M_PI, 3 * M_PI, -7.5, 100.0, 0.25};
        for (int k = 0; k < 6; ++k) S.add(k, 1, 0, 0, 1.0, in[k], w);
        for (int k = 0; k < 6; ++k) { const double zb = S.rec[(size_t)k * POLAR_REC + 1];
            CHECK(zb >= -M_PI && zb < M_PI && std::fabs(std::sin(zb) - std::sin(in[k])) < 1e-12 && std::fabs(std::cos(zb) - std::cos(in[k])) < 1e-12); }
        CHECK(S.rec[5 * POLAR_REC + 1] == 0.25);
    }
    {   // the upload rule
        PolarSync Y;
        CHECK(Y.needed(0, 0, 0, 0)); Y.done(3, 5, 7, 9);
        CHECK(!Y.needed(3, 5, 7, 9) && Y.needed(4, 5, 7, 9) && Y.needed(3, 6, 7, 9) && Y.needed(3, 5, 8, 9) && Y.needed(3, 5, 7, 10));
        Y.invalidate(); CHECK(Y.needed(3, 5, 7, 9));
    }
    std::printf("polar tables: ok\n");
    return 0;
}
