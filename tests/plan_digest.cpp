// plan_digest.cpp — characterisation of the host-side structure phase: one 64-bit FNV-1a digest per case over EVERY member of gs::Plan
// (declaration order; every vector's length and bytes, every scalar, every field of every Front; only ms_build is left out), after
// build_plan and, where a case grows, after grow_plan with the Growth record.  tests/golden/plan_digests.txt holds the output; a refactor
// of csrc/gs_plan.cpp must reproduce it byte for byte, at any number of host threads.  Its own main(), no HIP and no GPU:
//   g++ -std=c++17 -O2 -I opendlv-logic-cfsd18-sensation-slam_amd/csrc tests/plan_digest.cpp
//       opendlv-logic-cfsd18-sensation-slam_amd/csrc/gs_plan.cpp -o plan_digest -lpthread && ./plan_digest
//   --members     one digest per member instead of one per plan: a mismatch names the array
//   --capacities  the capacities of the arrays grow_plan appends to, per successful world-1 build (not part of the golden file)
// Every case is built twice: fresh, and again on ONE Plan object with ONE workspace (large and small graphs alternating), where each
// digest must equal the fresh one; last, a grown plan is rebuilt there at equal counts.  The properties that make a case reach its branch are asserted here.
#include "gs_host.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>

using namespace gs;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

// ---------------------------------------------------------------- digest
struct Fnv {
    uint64_t h = 14695981039346656037ull;
    void bytes(const void *p, size_t n) { const unsigned char *b = static_cast<const unsigned char *>(p); for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; } }
    template <class T> typename std::enable_if<std::is_arithmetic<T>::value>::type operator()(T v) { if (std::is_same<T, bool>::value) { const uint8_t b = v ? 1 : 0; bytes(&b, 1); } else bytes(&v, sizeof v); }
    template <class T, class A> typename std::enable_if<std::is_arithmetic<T>::value>::type operator()(const std::vector<T, A> &v) { (*this)((uint64_t)v.size()); bytes(v.data(), v.size() * sizeof(T)); }
    template <class A> void operator()(const std::vector<AsmRec, A> &v) { (*this)((uint64_t)v.size()); for (const AsmRec &r : v) { (*this)(r.kind); (*this)(r.src); (*this)(r.r0); (*this)(r.c0); } }
    void operator()(const std::vector<Front> &v) { (*this)((uint64_t)v.size());      // (field by field: the struct has padding)
        for (const Front &F : v) { (*this)(F.npiv); (*this)(F.nbnd); (*this)(F.piv0); (*this)(F.parent); (*this)(F.level); (*this)(F.owner); (*this)(F.opaque);
            (*this)(F.bnd_off); (*this)(F.map_off); (*this)(F.L_off); (*this)(F.U_off); (*this)(F.asm_off); (*this)(F.asm_cnt); (*this)(F.asm_dup); (*this)(F.child_off); (*this)(F.child_cnt); } }
};
// every member of Plan, declaration order (gs_host.hpp); ms_build is a wall time
template <class V> void visit_plan(const Plan &P, V &&v) {
#define M(x) v(#x, P.x)
    M(valid); M(n_scalar); M(pose_gidx); M(lm_gidx); M(pl_order); M(pp_order); M(pl_start); M(lm_start); M(lm_edges); M(ppadj_start); M(ppadj);
    M(ell_T); M(ell_R); M(ell_len); M(ell_p0); M(ell_np); M(ell_ins); M(ell_of_ins); M(ppinc); M(lin_ell_ok); M(n_wtiles); M(wt_lo); M(wt_hi);
    M(wt_grp_start); M(wt_desc); M(grp_lm); M(grp_pos_start); M(grp_pos); M(ell_dst); M(lm_grp_start); M(grp_slot); M(fronts); M(bnd_rows); M(child_map);
    M(children); M(asm_recs); M(level_start); M(level_fronts); M(max_front); M(l_doubles); M(u_doubles); M(factor_flops); M(world); M(rank);
    M(n_shared_fronts); M(dist); M(exchange_doubles); M(pl_rank); M(pp_rank); M(pose_known); M(lm_known); M(level_start_owned); M(level_fronts_owned);
    M(level_start_shared); M(level_fronts_shared); M(x_off); M(base_N); M(base_M); M(base_Epp); M(base_Epl); M(planned_N); M(planned_M); M(planned_Epp);
    M(planned_Epl); M(n_growths); M(root_f0); M(front_limit); M(reshape_version);
#undef M
}
template <class V> void visit_growth(const Growth &G, V &&v) {
#define M(x) v("growth." #x, G.x)
    M(fronts); M(bnd_from); M(map_from); M(asm_from); M(first_pose); M(first_lm); M(first_pp); M(first_pl);
#undef M
}
static bool g_members = false, g_caps = false;
// one line (or, --members, one per member) for `name`; returns the plan's digest.  `print` = false: the digest only (the recycled builds)
static uint64_t digest(const std::string &name, const Plan &P, const Growth *G, bool print) {
    Fnv all;
    auto one = [&](const char *member, const auto &x) { all(x);
        if (print && g_members) { Fnv m; m(x); std::printf("%s %s %016llx\n", name.c_str(), member, (unsigned long long)m.h); } };
    visit_plan(P, one);
    if (G) visit_growth(*G, one);
    if (print && !g_members) std::printf("%s %016llx\n", name.c_str(), (unsigned long long)all.h);
    return all.h;
}

// ---------------------------------------------------------------- graphs (the shapes of tests/upload_tables_san.cpp)
static void add_pose(HostGraph &g, bool fixed) { const int p = g.n_poses(); g.pose_id.push_back(p); g.pose_fixed.push_back(fixed); g.pose_est.insert(g.pose_est.end(), {0.1 * p, 0.0, 0.01 * p}); }
static void add_lm(HostGraph &g, bool fixed) { g.lm_id.push_back(g.n_lms()); g.lm_fixed.push_back(fixed); g.lm_est.insert(g.lm_est.end(), {0.5 * g.n_lms(), 1.0}); }
static void add_pp(HostGraph &g, int i, int j) { g.pp_i.push_back(i); g.pp_j.push_back(j); g.pp_z.insert(g.pp_z.end(), {0.1 * (j - i), 0.0, 0.01}); g.pp_info.insert(g.pp_info.end(), {1, 0, 0, 1, 0, 1}); }
static void add_pl(HostGraph &g, int p, int l) { g.pl_p.push_back(p); g.pl_l.push_back(l); g.pl_z.insert(g.pl_z.end(), {1.0, 0.25 * l}); g.pl_info.insert(g.pl_info.end(), {1, 0, 1}); }

// a chain of poses, pose 0 fixed, each seeing `views` consecutive landmarks that move along the chain; the last landmark fixed.
// chain(160, 39): pose p sees landmarks min(p * 38 / 160, 36) + {0, 1, 2} — the slope of upload_tables_san's chain
struct Chain { int n_poses, n_lms, views;
    int first_lm(int p) const { return (int)std::min<int64_t>((int64_t)p * (n_lms - 1) / n_poses, n_lms - views); }
    void pose(HostGraph &g, bool fixed = false) const { const int p = g.n_poses(); add_pose(g, p == 0 || fixed); if (p > 0) add_pp(g, p - 1, p); for (int j = 0; j < views; ++j) add_pl(g, p, first_lm(p) + j); } };
static HostGraph chain(int n_poses, int n_lms, int views = 3, int also_fixed = -1) {
    const Chain c{n_poses, n_lms, views}; HostGraph g;
    for (int l = 0; l < n_lms; ++l) add_lm(g, l == n_lms - 1);
    for (int p = 0; p < n_poses; ++p) c.pose(g, p == also_fixed);
    return g;
}
// 20 mutually connected free poses and a fixed one connected to all of them, two landmarks seen by every pose: a root front of 64 scalars
static HostGraph clique20_2lm() {
    HostGraph g;
    for (int p = 0; p < 21; ++p) add_pose(g, p == 0);
    for (int a = 0; a < 21; ++a) for (int b = a + 1; b < 21; ++b) add_pp(g, a, b);
    for (int l = 0; l < 2; ++l) { add_lm(g, false); for (int p = 0; p < 21; ++p) add_pl(g, p, l); }
    return g;
}
// the chain with one pose that sees `n` landmarks more
static HostGraph one_wide_pose(int n_poses, int n_lms, int at, int n) {
    HostGraph g; const Chain c{n_poses, n_lms, 3};
    for (int l = 0; l < n_lms; ++l) add_lm(g, l == n_lms - 1);
    for (int p = 0; p < n_poses; ++p) { c.pose(g); if (p == at) for (int l = 0, k = 0; k < n && l < n_lms; ++l) if (l < c.first_lm(p) || l >= c.first_lm(p) + 3) { add_pl(g, p, l); ++k; } }
    return g;
}
// chain(160, 39) with the observation edges inserted landmark-major, two exactly parallel observation edges, two parallel odometry edges and
// an odometry edge joining poses 10 and 150
static HostGraph shuffled() {
    HostGraph c = chain(160, 39), g = c;
    g.pl_p.clear(); g.pl_l.clear(); g.pl_z.clear(); g.pl_info.clear();
    for (int l = 0; l < c.n_lms(); ++l) for (int k = 0; k < c.n_pl(); ++k) if (c.pl_l[k] == l) add_pl(g, c.pl_p[k], l);
    add_pl(g, 50, c.pl_l[3 * 50]); add_pp(g, 70, 71); add_pp(g, 10, 150);
    return g;
}
static HostGraph nothing_free() { HostGraph g; add_pose(g, true); add_pose(g, true); add_pp(g, 0, 1); add_lm(g, true); add_pl(g, 1, 0); return g; }

// PlanOptions::lm_seen_interior / lm_seen_first by brute force from their definition: per landmark (insertion index) the windows whose interior
// poses / whose first pose see it; window of the f-th free pose = f * W / (free poses), a window's first pose = its lowest position (windows 1 ..)
static void brute_masks(const HostGraph &g, int W, std::vector<uint64_t> &interior, std::vector<uint64_t> &first) {
    std::vector<int> fp(g.n_poses(), -1); int nfp = 0;
    for (int p = 0; p < g.n_poses(); ++p) if (!g.pose_fixed[p]) fp[p] = nfp++;
    auto win = [&](int f) { return (int)((int64_t)f * W / nfp); };
    interior.assign(g.n_lms(), 0); first.assign(g.n_lms(), 0);
    for (int k = 0; k < g.n_pl(); ++k) { const int f = fp[g.pl_p[k]]; if (f < 0 || g.lm_fixed[g.pl_l[k]]) continue;
        const int w = win(f); const bool is_first = w >= 1 && (f == 0 || win(f - 1) != w);
        (is_first ? first : interior)[g.pl_l[k]] |= 1ull << w; }
}

// ---------------------------------------------------------------- cases
struct Case {
    std::string name; HostGraph g; PlanOptions o;
    bool masks = false;                                   // lm_seen_* handed over (filled in by run: the vectors live here)
    std::vector<uint64_t> seen_i, seen_f;
    std::function<void(const Plan &)> property;           // what makes the case reach its branch
    bool grows = false;                                   // case 1: two accepted growth steps, then refusals
    bool expect_error = false;
    uint64_t fresh = 0, fresh_grown = 0;
};
static int n_roots_of(const Plan &P, int rank) {         // subtrees of `rank`: its fronts whose parent is not its own
    int n = 0; for (const Front &F : P.fronts) n += F.owner == rank && !F.opaque && (F.parent < 0 || P.fronts[F.parent].owner != rank); return n; }

static void check_capacities(const std::string &name, const Plan &P) {
    if (P.world != 1) return;
    auto room = [](const auto &v) { return (int64_t)v.capacity() - (int64_t)v.size(); };
    CHECK(room(P.pose_gidx) >= TAIL_POSES && room(P.pose_known) >= TAIL_POSES && room(P.lm_gidx) >= TAIL_LMS && room(P.lm_known) >= TAIL_LMS);
    CHECK(room(P.pl_order) >= TAIL_PL && room(P.ell_of_ins) >= TAIL_PL && room(P.pl_rank) >= TAIL_PL && room(P.ell_ins) >= TAIL_PL);
    CHECK(room(P.pp_order) >= TAIL_PP && room(P.pp_rank) >= TAIL_PP);
    CHECK(room(P.bnd_rows) >= 64 * 1024 && room(P.child_map) >= 64 * 1024 && room(P.asm_recs) >= 96 * 1024);
    if (g_caps) std::printf("%s capacities: %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", name.c_str(), P.pose_gidx.capacity(), P.pose_known.capacity(), P.lm_gidx.capacity(),
                            P.lm_known.capacity(), P.pl_order.capacity(), P.ell_of_ins.capacity(), P.pl_rank.capacity(), P.ell_ins.capacity(), P.pp_order.capacity(), P.pp_rank.capacity(),
                            P.bnd_rows.capacity(), P.child_map.capacity(), P.asm_recs.capacity());
}

// growth of case 1: 4 appended poses in two steps (the second with a landmark of its own) must be accepted; then batches that must be refused
// without a byte of the plan changing
static uint64_t grow(Case &c, Plan &P, bool print) {
    HostGraph g = c.g; const Chain ch{160, 39, 3}; uint64_t d = 0;
    for (int step = 0; step < 2; ++step) {
        ch.pose(g); ch.pose(g);
        if (step == 1) { add_lm(g, false); add_pl(g, g.n_poses() - 2, g.n_lms() - 1); add_pl(g, g.n_poses() - 1, g.n_lms() - 1); }
        Growth gr; std::string why;
        if (!grow_plan(g, P, gr, why)) { std::fprintf(stderr, "%s: grow_plan refused: %s\n", c.name.c_str(), why.c_str()); std::exit(1); }
        CHECK(P.n_growths == step + 1 && P.planned_N == 162 + 2 * step);
        d = digest(c.name + "+grow" + std::to_string(step + 1), P, &gr, print);
    }
    const uint64_t before = digest("", P, nullptr, false);
    auto refused = [&](const char *what, HostGraph h) { Growth gr; std::string why;
        CHECK(!grow_plan(h, P, gr, why) && digest("", P, nullptr, false) == before);
        if (print) std::printf("%s+refuse:%s \"%s\"\n", c.name.c_str(), what, why.c_str()); };
    { HostGraph h = g; for (int k = 0; k < TAIL_POSES; ++k) ch.pose(h); refused("17-poses", h); }
    { HostGraph h = g; add_pl(h, 5, 1); refused("old-pose-edge", h); }
    { HostGraph h = g; for (int k = 0; k < 12; ++k) { add_pose(h, false); add_pp(h, 1 + 13 * k, h.n_poses() - 1); }      // (the root would gain 36 + 30 scalars)
      for (int k = 0; k < 15; ++k) { add_lm(h, false); add_pl(h, h.n_poses() - 1 - k % 12, h.n_lms() - 1); } refused("full-front", h); }
    return d;
}

// one build of a case into P (fresh or recycled)
static uint64_t run(Case &c, Plan &P, std::shared_ptr<void> *ws, bool print, uint64_t *grown) {
    PlanOptions o = c.o;
    if (c.masks) { brute_masks(c.g, o.world, c.seen_i, c.seen_f); o.lm_seen_interior = c.seen_i.data(); o.lm_seen_first = c.seen_f.data(); }
    std::string err;
    const bool ok = build_plan(c.g, o, P, err, ws);
    if (!ok) { CHECK(c.expect_error); if (print) std::printf("%s error \"%s\"\n", c.name.c_str(), err.c_str());
        Fnv f; f.bytes(err.data(), err.size()); return f.h; }
    CHECK(!c.expect_error && P.valid);
    if (c.property) c.property(P);
    check_capacities(c.name, P);
    const uint64_t d = digest(c.name, P, nullptr, print);
    if (c.grows) *grown = grow(c, P, print);
    return d;
}

int main(int argc, char **argv) {
    for (int a = 1; a < argc; ++a) { if (!std::strcmp(argv[a], "--members")) g_members = true; else if (!std::strcmp(argv[a], "--capacities")) g_caps = true; else { std::fprintf(stderr, "usage: plan_digest [--members] [--capacities]\n"); return 2; } }
    std::vector<Case> cases;
    auto add = [&](std::string name, HostGraph g, PlanOptions o = PlanOptions()) -> Case & { cases.emplace_back(); Case &c = cases.back(); c.name = std::move(name); c.g = std::move(g); c.o = o; return c; };
    auto opts = [](auto &&set) { PlanOptions o; set(o); return o; };
    const HostGraph c1 = chain(160, 39);
    // 1: wave fronts only; grown
    { Case &c = add("01-chain160", c1); c.grows = true; c.property = [](const Plan &P) { CHECK(P.max_front <= 63 && P.lin_ell_ok && !P.dist); }; }
    // 2: the first workgroup front: the size-class sort of the levels
    add("02-clique20", clique20_2lm()).property = [](const Plan &P) { CHECK(P.max_front == 64); };
    // 3: wide view (16 landmarks per pose): workgroup cluster fronts, leaves of 8, no headroom
    add("03-wide16", chain(400, 116, 16)).property = [](const Plan &P) { CHECK(P.max_front > 63); };
    // 4: a pose with 33 observations: past the fused layout
    add("04-pose33", one_wide_pose(40, 40, 20, 30)).property = [](const Plan &P) { CHECK(!P.lin_ell_ok && P.ell_T == 8 && P.ell_R == 5); };
    // 5: observation edges not grouped by pose (the counting sort), parallel edges, an odometry edge across the chain
    add("05-shuffled", shuffled()).property = [](const Plan &P) { int dup = 0; for (const Front &F : P.fronts) dup += F.asm_dup; CHECK(dup > 0); bool id = true; for (size_t k = 0; k < P.pl_order.size(); ++k) id = id && P.pl_order[k] == (int32_t)k; CHECK(!id); };
    // 6: leaf size by the graph: 100 free poses -> leaves of 6, 120 -> leaves of 8 (asserted below: the digests of the explicit sizes)
    for (int n : {101, 121}) for (int leaf : {0, 6, 8}) add("06-leaf-n" + std::to_string(n) + "-leaf" + std::to_string(leaf), chain(n, n / 4), opts([&](PlanOptions &o) { o.leaf_poses = leaf; }));
    add("06-leaf-n101-leaf3", chain(101, 25), opts([](PlanOptions &o) { o.leaf_poses = 3; }));
    add("06-leaf-n101-ways2", chain(101, 25), opts([](PlanOptions &o) { o.leaf_poses = 0; o.cluster_ways = 2; }));
    // 7: lanes per pose
    for (int T : {1, 2, 4, 8}) add("07-lanes" + std::to_string(T), c1, opts([&](PlanOptions &o) { o.ell_lanes = T; })).property = [T](const Plan &P) { CHECK(P.ell_T == T); };
    // 8: world 8, every rank: by windows, by the general recursion, and with the masks handed over
    const HostGraph c8 = chain(257, 65);
    for (int r = 0; r < 8; ++r) {
        add("08-w8-r" + std::to_string(r) + "-windows", c8, opts([&](PlanOptions &o) { o.world = 8; o.rank = r; })).property = [](const Plan &P) { bool minus = false; for (int32_t v : P.pl_rank) minus = minus || v == -1; CHECK(P.dist && minus); };
        add("08-w8-r" + std::to_string(r) + "-general", c8, opts([&](PlanOptions &o) { o.world = 8; o.rank = r; o.by_window = false; })).property = [](const Plan &P) { for (int32_t v : P.pl_rank) CHECK(v >= 0); };
        add("08-w8-r" + std::to_string(r) + "-masks", c8, opts([&](PlanOptions &o) { o.world = 8; o.rank = r; })).masks = true; }
    // 9: an odometry edge between the interiors of two windows: the general recursion; with masks an error
    { HostGraph g = c8; add_pp(g, 40, 100);
      for (int r : {0, 3}) add("09-w8-r" + std::to_string(r) + "-interior-edge", g, opts([&](PlanOptions &o) { o.world = 8; o.rank = r; })).property = [](const Plan &P) { for (int32_t v : P.pl_rank) CHECK(v >= 0); };
      Case &c = add("09-w8-r3-interior-edge-masks", g, opts([](PlanOptions &o) { o.world = 8; o.rank = 3; })); c.masks = true; c.expect_error = true; }
    // 10: a fixed pose inside rank 3's window (one landmark per pose; the pose behind the fixed one is a split pose of the window's cluster): the
    // window falls into several subtrees, the shared fronts get the range's boundary as a whole
    { const HostGraph g = chain(257, 65, 1, 105);
      for (int r = 0; r < 8; ++r) { Case &c = add("10-w8-r" + std::to_string(r) + "-fixed-inside", g, opts([&](PlanOptions &o) { o.world = 8; o.rank = r; }));
          if (r == 3) c.property = [](const Plan &P) { CHECK(n_roots_of(P, 3) > 1); }; } }
    // 11: a forced shared top on one rank
    add("11-shared-top2", c1, opts([](PlanOptions &o) { o.force_shared_top = 2; })).property = [](const Plan &P) { CHECK(P.dist && P.world == 1 && P.n_shared_fronts > 0 && P.exchange_doubles > 2); };
    // 12: no free vertex
    add("12-nothing-free", nothing_free()).expect_error = true;
    // 13: large enough for every region of the build to run in several parts on the host threads
    { const HostGraph g = chain(40000, 10000);
      add("13-chain40000", g);
      add("13-chain40000-w8-r3", g, opts([](PlanOptions &o) { o.world = 8; o.rank = 3; })); }

    for (Case &c : cases) { Plan P; c.fresh = run(c, P, nullptr, true, &c.fresh_grown); }
    auto by_name = [&](const char *n) -> Case & { for (Case &c : cases) if (c.name == n) return c; std::fprintf(stderr, "no case %s\n", n); std::exit(1); };
    CHECK(by_name("06-leaf-n101-leaf0").fresh == by_name("06-leaf-n101-leaf6").fresh && by_name("06-leaf-n101-leaf0").fresh != by_name("06-leaf-n101-leaf8").fresh);
    CHECK(by_name("06-leaf-n121-leaf0").fresh == by_name("06-leaf-n121-leaf8").fresh && by_name("06-leaf-n121-leaf0").fresh != by_name("06-leaf-n121-leaf6").fresh);
    CHECK(by_name("07-lanes4").fresh != by_name("07-lanes2").fresh);
    for (int r = 0; r < 8; ++r) { const std::string n = "08-w8-r" + std::to_string(r);      // masks handed over = masks computed here: the same plan
        CHECK(by_name((n + "-masks").c_str()).fresh == by_name((n + "-windows").c_str()).fresh && by_name((n + "-general").c_str()).fresh != by_name((n + "-windows").c_str()).fresh); }

    // 14: every case again on one Plan object with one workspace, large and small graphs alternating
    std::vector<int> order(cases.size()), alt;
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cases[a].g.n_poses() > cases[b].g.n_poses(); });
    for (size_t lo = 0, hi = order.size(); lo < hi;) { alt.push_back(order[lo++]); if (lo < hi) alt.push_back(order[--hi]); }
    Plan P; std::shared_ptr<void> ws;
    for (int i : alt) { Case &c = cases[i]; uint64_t grown = 0;
        const uint64_t d = run(c, P, &ws, false, &grown);
        if (d != c.fresh || grown != c.fresh_grown) { std::fprintf(stderr, "%s: the recycled build differs from the fresh one\n", c.name.c_str()); return 1; } }
    std::printf("14-recycled %zu builds equal their fresh digests\n", alt.size());
    // 15: a grown plan rebuilt at equal counts on its own Plan and workspace — a loop-closure odometry edge between old poses: grow_plan refuses, the
    // full build takes over, and every recycled array already has the size it needs (and no more capacity than the first build gave it): the digest of
    // a fresh build, and the room grow_plan needs
    { Case &c = by_name("01-chain160"); HostGraph g = c.g; const Chain ch{160, 39, 3}; std::string err, why; Plan Q; std::shared_ptr<void> wq;
      CHECK(build_plan(g, c.o, Q, err, &wq));
      for (int step = 0; step < 3; ++step) { ch.pose(g); ch.pose(g); Growth gr; CHECK(grow_plan(g, Q, gr, why)); }
      add_pp(g, 10, 150);
      { Growth gr; CHECK(!grow_plan(g, Q, gr, why) && why == "new odometry edge between old poses"); }
      CHECK((int)Q.pl_order.size() == g.n_pl() && (int)Q.pl_order.capacity() < g.n_pl() + TAIL_PL);
      CHECK(build_plan(g, c.o, Q, err, &wq)); check_capacities("15-regrown-at-equal-counts", Q);
      Plan F; CHECK(build_plan(g, c.o, F, err));
      CHECK(digest("15-regrown-at-equal-counts", Q, nullptr, true) == digest("", F, nullptr, false)); }
    return 0;
}
