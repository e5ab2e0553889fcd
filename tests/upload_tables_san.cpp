// upload_tables_san.cpp — stand-alone check of the tables a plan's upload and its append-only growth send to the device
// (csrc/gs_layout.hpp: the arena parts, Sc3Args, the patch slots; csrc/gs_upload_host.hpp: the builders that upload_graph and
// upload_growth share), on real plans from build_plan / grow_plan, against brute-force restatements written here.  Its own main(), no
// HIP and no GPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I opendlv-logic-cfsd18-sensation-slam_amd/csrc
//       tests/upload_tables_san.cpp opendlv-logic-cfsd18-sensation-slam_amd/csrc/gs_plan.cpp -o upload_tables_san -lpthread && ./upload_tables_san
#include "gs_upload_host.hpp"

#include <cstdio>
#include <cstdlib>
#include <set>

using namespace gs;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

static void add_pose(HostGraph &g, bool fixed, double x, double y, double th) {
    g.pose_id.push_back(g.n_poses()); g.pose_fixed.push_back(fixed); g.pose_est.insert(g.pose_est.end(), {x, y, th});
}
static void add_lm(HostGraph &g, bool fixed) { g.lm_id.push_back(g.n_lms()); g.lm_fixed.push_back(fixed); g.lm_est.insert(g.lm_est.end(), {0.5 * g.n_lms(), 1.0}); }
static void add_pp(HostGraph &g, int i, int j) {
    g.pp_i.push_back(i); g.pp_j.push_back(j); g.pp_z.insert(g.pp_z.end(), {0.1 * (j - i), -0.03 * j, 2.9 + 0.07 * j});        // (angles on both sides of pi)
    g.pp_info.insert(g.pp_info.end(), {1, 0, 0, 1, 0, 1});
}
static void add_pl(HostGraph &g, int p, int l) { g.pl_p.push_back(p); g.pl_l.push_back(l); g.pl_z.insert(g.pl_z.end(), {1.0, 0.25 * l}); g.pl_info.insert(g.pl_info.end(), {1, 0, 1}); }

// a chain of poses, pose 0 fixed, each seeing three consecutive landmarks that move along the chain; landmark 38 fixed
static int chain_first_lm(int p) { return std::min(p * 38 / 160, 37); }
static void chain_pose(HostGraph &g) {
    const int p = g.n_poses(); add_pose(g, p == 0, 0.1 * p, 0.0, 0.01 * p);
    if (p > 0) add_pp(g, p - 1, p);
    for (int j = 0; j < 3; ++j) add_pl(g, p, chain_first_lm(p) + j);
}
static HostGraph chain(int n_poses, int n_lms) {
    HostGraph g;
    for (int l = 0; l < n_lms; ++l) add_lm(g, l == 38);
    for (int p = 0; p < n_poses; ++p) chain_pose(g);
    return g;
}
// tests/shape_graphs.py, clique(20, 2): 20 mutually connected free poses and a fixed one connected to all of them, two landmarks seen by
// every pose — a root front of 64 scalars, the first workgroup front
static HostGraph clique20_2lm() {
    HostGraph g;
    for (int p = 0; p < 21; ++p) add_pose(g, p == 0, 1.0 * p, 2.0, 0.0);
    for (int a = 0; a < 21; ++a) for (int b = a + 1; b < 21; ++b) add_pp(g, a, b);
    for (int l = 0; l < 2; ++l) { add_lm(g, false); for (int p = 0; p < 21; ++p) add_pl(g, p, l); }
    return g;
}
static Plan plan_of(const HostGraph &g, int world = 1, int rank = 0) {
    PlanOptions o; o.world = world; o.rank = rank;
    Plan P; std::string err;
    if (!build_plan(g, o, P, err)) { std::fprintf(stderr, "build_plan: %s\n", err.c_str()); std::exit(1); }
    return P;
}

// ---------------------------------------------------------------- the arena
static void check_arena(const ArenaCounts &c) {
    ArenaOffsets o;
    CHECK(arena_layout(c, o));
    const int64_t want[ARENA_PARTS] = {6 * c.N, 3 * c.N, 9 * c.Epp, 6 * c.ell_len, 8 * c.n_groups, 3 * c.M, 2 * c.M,
                                       6 * c.tcapN, 3 * c.tcapN, 9 * c.tcapEpp, 6 * c.tcapEpl, 3 * c.tcapM, 2 * c.tcapM};
    CHECK(o.at[0] == 0 && ARENA_PARTS == 13 && ARENA_TAIL == 7);
    for (int k = 0; k < ARENA_PARTS; ++k) {
        CHECK(o.at[k] % 2 == 0);                                     // 16 bytes
        CHECK(o.at[k + 1] >= o.at[k] + want[k]);                     // large enough, ordered, disjoint
        CHECK(o.at[k + 1] <= o.at[k] + want[k] + 8); }               // ... and no more than the alignment asks for
    CHECK(o.at[ARENA_lm_part] % 8 == 0);                             // one 64-byte line per partial-sum record
    CHECK(o.at[ARENA_b_pose] == o.at[ARENA_Hpp_diag] + 6 * c.N);     // Hpp_diag | b_pose: nine contiguous planes
    CHECK(o.doubles() == o.at[ARENA_PARTS]);
    const Sc3Args A = sc3_args(o, c, true), B = sc3_args(o, c, false);
    CHECK(A.fused == 1 && B.fused == 0 && A.L == c.ell_len && A.N == c.N && A.M == c.M && A.Epp == c.Epp);
    CHECK(A.off[ARENA_Hpp_diag] == o.at[ARENA_Hpp_diag] && A.off[ARENA_b_pose] == o.at[ARENA_b_pose] && A.off[ARENA_Hpp_off] == o.at[ARENA_Hpp_off] &&
          A.off[ARENA_Hpl] == o.at[ARENA_Hpl] && A.off[ARENA_lm_part] == o.at[ARENA_lm_part] && A.off[ARENA_Hll_diag] == o.at[ARENA_Hll_diag] && A.off[ARENA_b_lm] == o.at[ARENA_b_lm]);
    for (int k = ARENA_TAIL; k < ARENA_PARTS; ++k) CHECK(A.toff[k - ARENA_TAIL] == o.at[k]);
    CHECK(A.tcapN == c.tcapN && A.tcapEpp == c.tcapEpp && A.tcapEpl == c.tcapEpl && A.tcapM == c.tcapM);
    static_assert(sizeof(Sc3Args) == 8 * 8 + 8 + 4 * 4 + 6 * 8 + 4 * 4, "Sc3Args keeps its binary layout");
}
static ArenaCounts counts_of(const HostGraph &g, const Plan &P) {
    return ArenaCounts{g.n_poses(), g.n_pp(), P.ell_len, (int64_t)P.grp_lm.size(), g.n_lms(), TAIL_POSES, TAIL_PP, TAIL_PL, TAIL_LMS};
}

// ---------------------------------------------------------------- per-front tables of one plan, as upload_graph builds them
struct FrontTables { std::vector<int32_t> bf, u3_off, u3_size; int64_t used_U = 0, used_sc = 0; };
static FrontTables front_tables(const Plan &P, bool fused) {
    FrontTables T; const size_t S = P.fronts.size();
    T.bf.assign(BF_INTS * S, 0); T.u3_off.resize(S); T.u3_size.resize(S);
    int64_t lo = 0;
    for (size_t s = 0; s < S; ++s) { const RecCount c = front_record_count(P, P.fronts[s], fused);
        bf_row(P.fronts[s], c, T.used_sc, lo, &T.bf[BF_INTS * s]); T.used_sc += c.padded(); lo += c.nl;
        T.u3_off[s] = (int32_t)T.used_U; T.u3_size[s] = u3_slot_size(P.fronts[s].nbnd); T.used_U += u3_slot_advance(T.u3_size[s]); }
    return T;
}
static void check_front_tables(const Plan &P) {
    for (int fused = 0; fused < 2; ++fused) {
        const FrontTables T = front_tables(P, fused != 0);
        int64_t sc_end = 0, lm_end = 0, u_end = 0;
        for (size_t s = 0; s < P.fronts.size(); ++s) { const Front &F = P.fronts[s]; const int32_t *r = &T.bf[BF_INTS * s];
            // the assembly records expanded kind by kind: a diagonal block of dimension n is its lower triangle and its rhs, an off-diagonal one rows x columns
            int ns = 0, nl = 0;
            for (int t = F.asm_off; t < F.asm_off + F.asm_cnt - F.asm_dup; ++t) switch (P.asm_recs[t].kind) {
                case ASM_POSE_DIAG: ns += 3 * 4 / 2 + 3; break;
                case ASM_LM_DIAG: if (fused) ++nl; else ns += 2 * 3 / 2 + 2; break;
                case ASM_LM_DIAG_TAIL: ns += 2 * 3 / 2 + 2; break;
                case ASM_PP: case ASM_PP_T: ns += 3 * 3; break;
                case ASM_PL: case ASM_PL_T: ns += 3 * 2; break;
                default: CHECK(!"unknown record kind"); }
            const RecCount c = front_record_count(P, F, fused != 0);
            CHECK(c.ns == ns && c.nl == nl && c.padded() % 64 == 0 && c.padded() >= ns && c.padded() < ns + 64);
            CHECK(r[0] == F.asm_off && r[1] == F.asm_cnt - F.asm_dup && r[2] == F.npiv + F.nbnd && r[3] == sc_end && r[4] == c.padded() && r[5] == lm_end && r[6] == nl && r[7] == 0);
            sc_end += r[4]; lm_end += r[6];
            // the update matrix: rows 0 .. nbnd of the boundary block, row r' holding columns 0 .. min(r', nbnd - 1); two more doubles behind it
            int usz = 0; for (int rr = 0; rr <= F.nbnd; ++rr) usz += std::min(rr, F.nbnd - 1) + 1;
            CHECK(T.u3_size[s] == usz && T.u3_off[s] % 2 == 0 && T.u3_off[s] >= u_end);
            u_end = (int64_t)T.u3_off[s] + usz + 2; }
        CHECK(T.used_U >= u_end && T.used_U % 2 == 0 && T.used_sc == sc_end);
    }
}

// ---------------------------------------------------------------- growth: the patch records against the full builders on the grown plan
static void check_growth(const Plan &base, const Plan &grown, const Growth &gr) {
    const bool fused = true;                                         // (a plan grows only with the fused linearisation layout)
    const FrontTables B = front_tables(base, fused), F = front_tables(grown, fused);
    int64_t used_U = B.used_U, used_sc = B.used_sc;
    CHECK(!gr.fronts.empty());
    for (int s : gr.fronts) { int32_t r[PATCH_INTS];
        for (int32_t &v : r) v = 0x5a5a5a5a;
        patch_record(grown, s, fused, used_U, used_sc, B.bf[BF_INTS * (size_t)s + 5], r);
        const DevFront want = dev_front(grown.fronts[(size_t)s]);
        CHECK(r[PATCH_FRONT] == s && std::memcmp(r + PATCH_DEVFRONT, &want, sizeof(want)) == 0);
        CHECK(r[PATCH_U3_OFF] == used_U && r[PATCH_U3_SIZE] == F.u3_size[(size_t)s] && r[PATCH_SPARE] == 0);
        for (int c = 0; c < BF_INTS; ++c) if (c != 3) CHECK(r[PATCH_BF + c] == F.bf[BF_INTS * (size_t)s + c]);       // (the landmark records stay where they are)
        CHECK(r[PATCH_BF + 6] == B.bf[BF_INTS * (size_t)s + 6]);    // growth adds no landmark-diagonal record: the front's landmark records are the base plan's
        CHECK(r[PATCH_BF + 3] == used_sc);                           // only the offsets that growth assigns behind the used room differ
        CHECK(used_U >= B.used_U && used_U % 2 == 0);
        used_U += u3_slot_advance(r[PATCH_U3_SIZE]); used_sc += r[PATCH_BF + 4]; }
    // a front that growth does not report keeps every row
    std::set<int> changed(gr.fronts.begin(), gr.fronts.end());
    for (size_t s = 0; s < base.fronts.size(); ++s) if (!changed.count((int)s)) {
        const DevFront a = dev_front(base.fronts[s]), b = dev_front(grown.fronts[s]);
        CHECK(std::memcmp(&a, &b, sizeof(a)) == 0 && B.u3_size[s] == F.u3_size[s]);
        for (int c = 0; c < BF_INTS; ++c) if (c != 3) CHECK(B.bf[BF_INTS * s + c] == F.bf[BF_INTS * s + c]); }
    // DevFront mirrors Front field by field
    for (const Front &f : grown.fronts) { const DevFront o = dev_front(f);
        CHECK(o.npiv == f.npiv && o.nbnd == f.nbnd && o.piv0 == f.piv0 && o.parent == f.parent && o.asm_off == f.asm_off && o.asm_cnt == f.asm_cnt && o.asm_dup == f.asm_dup &&
              o.child_off == f.child_off && o.child_cnt == f.child_cnt && o.owner == f.owner && o.level == f.level && o.pad0 == 0 && o.bnd_off == f.bnd_off &&
              o.map_off == f.map_off && o.L_off == f.L_off && o.U_off == f.U_off); }
}

// ---------------------------------------------------------------- the tail's groupings
static void check_tail_groups(const HostGraph &g, const Plan &P) {
    TailGroups T; tail_groups(g, P, T);
    const int tN = P.planned_N - P.base_N, tE = P.planned_Epl - P.base_Epl;
    CHECK((int)T.pose_start.size() == tN + 1 && T.pose_start[0] == 0 && T.pose_start[(size_t)tN] == tE && (int)T.pose_edges.size() == tE);
    std::vector<int> seen((size_t)tE, 0);
    for (int t = 0; t < tN; ++t) for (int q = T.pose_start[(size_t)t]; q < T.pose_start[(size_t)t + 1]; ++q) { const int e = T.pose_edges[(size_t)q];
        CHECK(e >= 0 && e < tE && g.pl_p[(size_t)(P.base_Epl + e)] == P.base_N + t && ++seen[(size_t)e] == 1);
        CHECK(q == T.pose_start[(size_t)t] || T.pose_edges[(size_t)q - 1] < e); }                 // edge order within a group
    for (int e = 0; e < tE; ++e) CHECK(seen[(size_t)e] == 1);
    int n_free = 0; for (int e = 0; e < tE; ++e) n_free += !g.lm_fixed[(size_t)g.pl_l[(size_t)(P.base_Epl + e)]];
    CHECK(T.lt_start.size() == T.lt_id.size() + 1 && T.lt_start[0] == 0 && T.lt_start.back() == n_free && (int)T.lt_edges.size() == n_free);
    std::fill(seen.begin(), seen.end(), 0);
    for (size_t j = 0; j < T.lt_id.size(); ++j) { const int l = T.lt_id[j];
        CHECK(!g.lm_fixed[(size_t)l] && (j == 0 || T.lt_id[j - 1] < l) && T.lt_start[j] < T.lt_start[j + 1]);
        for (int q = T.lt_start[j]; q < T.lt_start[j + 1]; ++q) { const int e = T.lt_edges[(size_t)q];
            CHECK(e >= 0 && e < tE && g.pl_l[(size_t)(P.base_Epl + e)] == l && ++seen[(size_t)e] == 1);
            CHECK(q == T.lt_start[j] || T.lt_edges[(size_t)q - 1] < e); } }
    for (int e = 0; e < tE; ++e) CHECK(seen[(size_t)e] == (g.lm_fixed[(size_t)g.pl_l[(size_t)(P.base_Epl + e)]] ? 0 : 1));      // fixed cones are left out
}

// ---------------------------------------------------------------- tables that only the full upload builds
static void check_plan_tables(const HostGraph &g, const Plan &P) {
    // incidence records: the edge, or -1 where another rank evaluates it; the other endpoint and the role
    const std::vector<int32_t> inc = incidence_records(P);
    CHECK(inc.size() == P.ppinc.size() / 2);
    for (size_t q = 0; q < inc.size() / 2; ++q) { const int32_t k = P.ppinc[4 * q], role = P.ppinc[4 * q + 1];
        const bool other_rank = P.world > 1 && P.pp_rank[(size_t)k] != P.rank;
        CHECK(inc[2 * q] == (other_rank ? -1 : k));
        CHECK((int32_t)((uint32_t)inc[2 * q + 1] & 0x7fffffffu) == (role ? g.pp_i[(size_t)k] : g.pp_j[(size_t)k]) && (int32_t)((uint32_t)inc[2 * q + 1] >> 31) == role); }
    // the level list and its inverse
    const std::vector<int32_t> lf = level_list(P), pos = pos_of_front(P, lf);
    CHECK(lf.size() == P.level_fronts_owned.size() + P.level_fronts_shared.size() && pos.size() == P.fronts.size());
    for (size_t q = 0; q < lf.size(); ++q) { CHECK(lf[q] == (q < P.level_fronts_owned.size() ? P.level_fronts_owned[q] : P.level_fronts_shared[q - P.level_fronts_owned.size()]));
        CHECK(pos[(size_t)lf[q]] == (int32_t)q); }
    size_t listed = 0; for (int32_t v : pos) listed += v >= 0;
    CHECK(listed == lf.size());
    // children tables: one row table per child, 72 ints, or 168 when the plan holds a front of more than 63 scalars
    std::vector<int32_t> xrow;
    CHECK(children_row_offsets(P, lf, xrow) && xrow.size() == lf.size() + 1 && xrow[0] == 0 && f3x_stride(P) == (P.max_front > 63 ? 168 : 72));
    for (size_t q = 0; q < lf.size(); ++q) CHECK(xrow[q + 1] - xrow[q] == f3x_stride(P) * P.fronts[(size_t)lf[q]].child_cnt);
    const std::vector<int32_t> cd = child_desc(P);
    CHECK(cd.size() == 4 * P.children.size());
    for (size_t q = 0; q < P.children.size(); ++q) { const Front &C = P.fronts[(size_t)P.children[q]];
        CHECK(cd[4 * q] == P.children[q] && (cd[4 * q + 1] & 0xffff) == C.npiv && (cd[4 * q + 1] >> 16) == C.nbnd && cd[4 * q + 2] == C.owner && cd[4 * q + 3] == (int32_t)C.map_off); }
    // the group table: every group of this rank's wave tiles names its positions inside its tile and its slot
    if (P.lin_ell_ok) { const std::vector<int32_t> gt = group_table(P);
        CHECK(gt.size() == 2 * P.grp_slot.size() + 2);
        for (int w = P.wt_lo; w < P.wt_hi; ++w) { const int ga = P.wt_desc[4 * (size_t)w], gn = P.wt_desc[4 * (size_t)w + 1], p0 = P.wt_desc[4 * (size_t)w + 2], np = P.wt_desc[4 * (size_t)w + 3];
            for (int q = ga; q < ga + gn; ++q) { const int first = gt[2 * (size_t)q] & 0xffff, end = gt[2 * (size_t)q] >> 16;
                CHECK(first == P.grp_pos_start[(size_t)q] - p0 && end == P.grp_pos_start[(size_t)q + 1] - p0 && first < end && end <= np && gt[2 * (size_t)q + 1] == P.grp_slot[(size_t)q]); } } }
    // room behind the plan arrays: half the array, within its bounds
    CHECK(room_of(0, 8, 64) == 8 && room_of(40, 8, 64) == 20 && room_of(1000, 8, 64) == 64);
    CHECK(room_rows(P) >= 8 * 1024 && room_rows(P) <= 64 * 1024 && room_recs(P) >= 12 * 1024 && room_recs(P) <= 96 * 1024);
    const int64_t big = P.max_front > 63 ? 4 : 1;
    CHECK(room_U(P, 0) == (128 << 10) && room_U(P, (int64_t)1 << 30) == (big << 20) && room_sc(P, 0) == (64 << 10) && room_sc(P, (int64_t)1 << 30) == (big << 19));
    CHECK(room_L(P) >= (256 << 10) && room_L(P) <= (2 * big << 20));
    // the inverted odometry measurement: z^-1 composed with z is the identity; the angle in [-pi, pi) with its cos and sin
    for (int k = 0; k < g.n_pp(); ++k) { const double *z = &g.pp_z[3 * (size_t)k]; double o[5]; zinv5(z, o);
        const double c = std::cos(z[2]), s = std::sin(z[2]);
        CHECK(std::fabs(z[0] + c * o[0] - s * o[1]) < 1e-12 && std::fabs(z[1] + s * o[0] + c * o[1]) < 1e-12 && std::fabs(std::remainder(z[2] + o[2], 2 * M_PI)) < 1e-12);
        CHECK(o[2] >= -M_PI && o[2] < M_PI && o[3] == std::cos(o[2]) && o[4] == std::sin(o[2])); }
}

int main() {
    // ---- the arena on its own: odd counts (every part needs padding), nothing at all, and the 2^31 refusal
    check_arena(ArenaCounts{3, 1, 5, 3, 1, 1, 1, 1, 1});
    check_arena(ArenaCounts{0, 0, 0, 0, 0, TAIL_POSES, TAIL_PP, TAIL_PL, TAIL_LMS});
    { ArenaOffsets o; const int64_t L = (((int64_t)1 << 31) - 20000) / 6;
      CHECK(arena_layout(ArenaCounts{0, 0, L, 0, 0, TAIL_POSES, TAIL_PP, TAIL_PL, TAIL_LMS}, o) && o.doubles() < ((int64_t)1 << 31));
      CHECK(!arena_layout(ArenaCounts{0, 0, L + 20000, 0, 0, TAIL_POSES, TAIL_PP, TAIL_PL, TAIL_LMS}, o));
      CHECK(!arena_layout(ArenaCounts{(int64_t)1 << 28, 0, 0, 0, 0, 0, 0, 0, 0}, o) && arena_layout(ArenaCounts{((int64_t)1 << 28) / 9 * 8, 0, 0, 0, 0, 0, 0, 0, 0}, o)); }
    CHECK(PATCH_FRONT == 0 && PATCH_DEVFRONT == 1 && PATCH_U3_OFF == 21 && PATCH_U3_SIZE == 22 && PATCH_BF == 23 && PATCH_BF + BF_INTS == PATCH_SPARE && PATCH_INTS == 32);

    // ---- a chain of 160 poses and 40 landmarks, three views per pose: wave fronts only; grown by 4 poses in two steps, the second with
    // a landmark of its own
    {
        HostGraph g = chain(160, 40);
        const Plan base = plan_of(g);
        CHECK(base.max_front <= 63 && base.lin_ell_ok && !base.dist && base.base_N == 160);
        check_arena(counts_of(g, base)); check_front_tables(base); check_plan_tables(g, base);
        Plan P = base;
        for (int step = 0; step < 2; ++step) {
            const Plan before = P;
            chain_pose(g); chain_pose(g);
            if (step == 1) { add_lm(g, false); add_pl(g, g.n_poses() - 2, 40); add_pl(g, g.n_poses() - 1, 40); }
            Growth gr; std::string why;
            if (!grow_plan(g, P, gr, why)) { std::fprintf(stderr, "grow_plan refused: %s\n", why.c_str()); return 1; }
            CHECK(P.n_growths == step + 1 && P.planned_N == 162 + 2 * step && P.max_front <= 63);
            check_front_tables(P); check_growth(before, P, gr); check_tail_groups(g, P);
        }
        bool tail_lm = false; for (const AsmRec &a : P.asm_recs) tail_lm = tail_lm || a.kind == ASM_LM_DIAG_TAIL;
        CHECK(tail_lm && P.planned_M == 41 && P.planned_Epl - P.base_Epl == 14);
    }
    // ---- the smallest shape graph with a front of more than 63 scalars: 168-int children tables
    {
        const HostGraph g = clique20_2lm();
        const Plan P = plan_of(g);
        CHECK(P.max_front == 64 && f3x_stride(P) == 168);
        check_arena(counts_of(g, P)); check_front_tables(P); check_plan_tables(g, P);
    }
    // ---- the chain as rank 3 of 8 pose windows: incidence records of the other ranks' edges carry -1
    {
        const HostGraph g = chain(160, 40);
        const Plan P = plan_of(g, 8, 3);
        CHECK(P.world == 8 && P.rank == 3 && P.dist);
        int mine = 0, others = 0; for (int32_t r : P.pp_rank) (r == 3 ? mine : others)++;
        CHECK(mine > 0 && others > 0);
        const std::vector<int32_t> inc = incidence_records(P);
        int neg = 0; for (size_t q = 0; q < inc.size() / 2; ++q) neg += inc[2 * q] < 0;
        CHECK(neg > 0 && neg < (int)inc.size() / 2);
        check_arena(counts_of(g, P)); check_front_tables(P); check_plan_tables(g, P);
    }
    std::puts("upload tables: ok");
    return 0;
}
