// gs_schedule.cpp — build_schedule: the launch geometry of a plan, decided once with the plan; export_schedule: its flat record.
#include "gs_schedule.hpp"

#include <algorithm>

namespace gs {

// LDS needs of the front kernels (gs_kernels.hip; declared in gs_device.hpp, repeated here to keep this unit free of device headers)
size_t factor_sub_lds_bytes(int leaf_slot);
size_t factor_tab_lds_bytes(int kind);
size_t backsolve_tab_lds_bytes(int kind, int f_or_slot_f, int npiv_small);
int factor_lds_limit_f();

// ---- plans that hold a front of more than 63 scalars: the workgroup tables of the table-driven launches.  Factor: level positions
// upwards from the end of the leaf launch — a big front a workgroup (NT = 7 or 10 tile rows), a small front of the upper levels (the
// last block_n positions) four waves, other small fronts a wave each in groups of up to four that do not straddle a level.
// Backward solve: every position from the root downwards.
static void build_big_tables(const Plan &P, Schedule &S) {
    const LevelSet &ls = S.own; const int nlev = (int)ls.start.size() - 1, total = nlev > 0 ? ls.start[nlev] : 0;
    auto f_of = [&](int q) { const Front &F = P.fronts[P.level_fronts_owned[q]]; return F.npiv + F.nbnd; };
    auto big_kind = [&](int f) { return f <= 79 ? 4 : (f <= 111 ? 2 : 3); };        // 5, 7 or 10 tile rows
    S.small_max_npiv = 1; S.small_max_f = 1;
    for (const Front &F : P.fronts) if (!F.opaque && F.npiv + F.nbnd <= 63) { S.small_max_npiv = std::max(S.small_max_npiv, (int)F.npiv); S.small_max_f = std::max(S.small_max_f, F.npiv + F.nbnd); }
    auto push = [&](WgTable &t, int pos, int kind_cnt, int level, size_t lds, int cls) {
        const int e = (int)t.wg.size() / 2; t.wg.push_back(pos); t.wg.push_back(kind_cnt);
        if (!t.seg.empty() && t.seg.back().level == level && t.seg.back().lds == lds && t.seg.back().cls == cls) ++t.seg.back().count; else t.seg.push_back({e, 1, level, lds, cls}); };
    auto fcls = [](int kind) { return kind == 4 ? 0 : (kind == 3 ? 2 : 1); };       // factor kernel class: fronts of 64-79 | small fronts and 80-111 | 112-159
    const int first = S.leaf_n, first_block = total - S.block_n;
    for (int l = 0; l < nlev; ++l)
        for (int q = std::max(ls.start[l], first); q < ls.start[l + 1]; ) {
            const int f = f_of(q);
            if (f > 63) { const int k = big_kind(f); push(S.tab[TAB_F], q, k, l, factor_tab_lds_bytes(k), fcls(k)); ++q; }
            else if (q >= first_block) { push(S.tab[TAB_F], q, 1 | (1 << 8), l, factor_tab_lds_bytes(1), 1); ++q; }
            else { int cnt = 1; while (cnt < 4 && q + cnt < ls.start[l + 1] && q + cnt < first_block && f_of(q + cnt) <= 63) ++cnt;
                push(S.tab[TAB_F], q, 0 | (cnt << 8), l, factor_tab_lds_bytes(0), 1); q += cnt; } }
    for (int l = nlev - 1; l >= 0; --l)
        for (int q = ls.start[l + 1] - 1; q >= ls.start[l]; ) {
            const int f = f_of(q);
            if (f > 63) { // LDS by the size class of the front (the largest front of the class), so that runs of one class share a launch
                const int k = big_kind(f), fc = k == 4 ? 79 : (k == 2 ? 111 : 159);
                push(S.tab[TAB_B], q, k, l, backsolve_tab_lds_bytes(k, fc, 0), 1); --q; }
            else { int cnt = 1; while (cnt < 4 && q - cnt >= ls.start[l] && f_of(q - cnt) <= 63) ++cnt;
                push(S.tab[TAB_B], q, 0 | (cnt << 8), l, backsolve_tab_lds_bytes(0, S.small_max_f, S.small_max_npiv), 0); q -= cnt; } }
    // ---- pose-window shards: the SHARED top of a plan with workgroup fronts (round 4).  Three tables over the shared level positions
    // (shared_base + q): contributions (mode CONTRIB: no dependencies among them; a small front a wave — the four-wave form has no such
    // mode —, a big one a workgroup), the top itself (mode TOP, children first: a small front four waves, a big one a workgroup), and
    // the backward solve (root first).
    { const LevelSet &sh = S.shared; const int nls = (int)sh.start.size() - 1, B0 = S.shared_base;
      auto fs = [&](int q) { const Front &F = P.fronts[P.level_fronts_shared[q]]; return F.npiv + F.nbnd; };
      for (int l = 0; l < nls; ++l)
          for (int q = sh.start[l]; q < sh.start[l + 1]; ) { const int f = fs(q);
              if (f > 63) { const int k = big_kind(f);
                  push(S.tab[TAB_SC], B0 + q, k, l, factor_tab_lds_bytes(k), fcls(k)); push(S.tab[TAB_ST], B0 + q, k, l, factor_tab_lds_bytes(k), fcls(k)); ++q; }
              else { push(S.tab[TAB_ST], B0 + q, 1 | (1 << 8), l, factor_tab_lds_bytes(1), 1);
                  int cnt = 1; while (cnt < 4 && q + cnt < sh.start[l + 1] && fs(q + cnt) <= 63) ++cnt;
                  push(S.tab[TAB_SC], B0 + q, 0 | (cnt << 8), l, factor_tab_lds_bytes(0), 1);
                  for (int k2 = 1; k2 < cnt; ++k2) push(S.tab[TAB_ST], B0 + q + k2, 1 | (1 << 8), l, factor_tab_lds_bytes(1), 1);
                  q += cnt; } }
      for (int l = nls - 1; l >= 0; --l)
          for (int q = sh.start[l + 1] - 1; q >= sh.start[l]; ) { const int f = fs(q);
              if (f > 63) { const int k = big_kind(f), fc = k == 4 ? 79 : (k == 2 ? 111 : 159); push(S.tab[TAB_SB], B0 + q, k, l, backsolve_tab_lds_bytes(k, fc, 0), 1); --q; }
              else { int cnt = 1; while (cnt < 4 && q - cnt >= sh.start[l] && fs(q - cnt) <= 63) ++cnt;
                  push(S.tab[TAB_SB], B0 + q, 0 | (cnt << 8), l, backsolve_tab_lds_bytes(0, S.small_max_f, S.small_max_npiv), 0); q -= cnt; } } }
}

Schedule build_schedule(const Plan &P, const std::vector<int32_t> &pos_of_front, int factor_variant, bool tree_wanted, const gs_debug_options &opt) {
    Schedule S; S.factor_variant = factor_variant; S.big = factor_variant == 3 && P.max_front > 63;
    S.shared_base = (int)P.level_fronts_owned.size();
    // per-level launch parameters and the global workspace for fronts beyond the LDS limit
    const int nlev = (int)P.level_start.size() - 1;
    const int lim = factor_lds_limit_f();
    auto level_params = [&](const std::vector<int32_t> &start, const std::vector<int32_t> &list, LevelSet &ls) {
        ls.start = start; ls.max_f.assign(nlev, 0); ls.max_npiv.assign(nlev, 0); ls.max_nbnd.assign(nlev, 0);
        for (int l = 0; l < nlev; ++l) {
            for (int q = start[l]; q < start[l + 1]; ++q) { const Front &F = P.fronts[list[q]];
                ls.max_f[l] = std::max(ls.max_f[l], F.npiv + F.nbnd);
                ls.max_npiv[l] = std::max(ls.max_npiv[l], F.npiv); ls.max_nbnd[l] = std::max(ls.max_nbnd[l], F.nbnd); }
            if (ls.max_f[l] > lim) { const int64_t f = ls.max_f[l];
                S.front_ws_stride = std::max(S.front_ws_stride, ((f + 1) | 1) * f);
                S.ws_blocks = std::max<int64_t>(S.ws_blocks, start[l + 1] - start[l]); }
        }
    };
    level_params(P.level_start_owned, P.level_fronts_owned, S.own);
    level_params(P.level_start_shared, P.level_fronts_shared, S.shared);
    if (S.ws_blocks > 0) S.ws_blocks = std::max<int64_t>(S.ws_blocks, (int64_t)P.level_fronts_shared.size());      // one slice per block
    const LevelSet &ls = S.own;
    if (factor_variant == 3 && tree_wanted && nlev > 0) {
        // leaf instance: level 0 only if its fronts really have no children (always true for an elimination tree's level 0)
        { int n_leaf = ls.start[1], F_leaf_all = 0, slot = 256;
          // leaves beyond a wave (the fronts of a level are sorted by size class: the small ones first) go to the table-driven launch
          for (int q = 0; q < n_leaf; ++q) { const Front &F = P.fronts[P.level_fronts_owned[q]]; if (F.npiv + F.nbnd > 63) { n_leaf = q; break; } }
          for (int q = 0; q < n_leaf; ++q) { const Front &F = P.fronts[P.level_fronts_owned[q]];
              S.leaf_max_f = std::max(S.leaf_max_f, F.npiv + F.nbnd);
              if (F.child_cnt != 0) { n_leaf = 0; break; }
              slot = std::max(slot, (((F.npiv + F.nbnd + 1) | 1) * F.npiv + 1) & ~1); }
          F_leaf_all = n_leaf;                                        // GS_LEAF_KERNEL=2: leaf launches whatever their number
          // few leaves (all resident at once anyway: <= GS_LEAF_MIN, default 2048): no separate leaf launches, the whole-tree
          // launches take level 0 as well — two kernel boundaries less per iteration (cfg1-cfg3: 6-11 % of it)
          if (n_leaf <= opt.leaf_min) n_leaf = 0;
          if (opt.leaf_kernel == 0) n_leaf = 0; else if (opt.leaf_kernel == 2) n_leaf = F_leaf_all;
          S.leaf_n = n_leaf; S.leaf_slot = slot;
          // the bottom subtrees (k_factor3_sub): every level-1 front of this rank with the leaves below it in one workgroup — their update
          // matrices never leave the chip.  Taken when the leaf instance is in use, the plan put the leaves under
          // level-1 fronts behind the others (gs_plan.cpp) and the workgroup's LDS fits; the leaf launch then covers positions [0, sub_free).
          S.sub_n = 0; S.sub_first = 0; S.sub_free = n_leaf;
          if (opt.subtree != 0 && n_leaf > 0 && n_leaf == ls.start[1] && P.max_front <= 63 && nlev >= 2 &&
              factor_sub_lds_bytes(slot) <= (size_t)160 * 1024) {
              const auto &lfo = P.level_fronts_owned;
              auto under = [&](int s) { const int pa = P.fronts[s].parent; return pa >= 0 && P.fronts[pa].level == 1 && pos_of_front[pa] >= ls.start[1] && pos_of_front[pa] < ls.start[2]; };
              int nfree = 0; while (nfree < n_leaf && !under(lfo[nfree])) ++nfree;
              bool ok = true; int64_t kids = 0;
              for (int q = nfree; q < n_leaf && ok; ++q) ok = under(lfo[q]);
              for (int q = ls.start[1]; q < ls.start[2] && ok; ++q) { const Front &F = P.fronts[lfo[q]]; kids += F.child_cnt;
                  for (int c = 0; c < F.child_cnt && ok; ++c) { const int cp = pos_of_front[P.children[F.child_off + c]]; ok = cp >= nfree && cp < n_leaf; } }
              if (ok && kids == n_leaf - nfree && ls.start[2] > ls.start[1]) { S.sub_first = ls.start[1]; S.sub_n = ls.start[2] - ls.start[1]; S.sub_free = nfree; } } }
        // the upper levels — few fronts, all of them in the dependent chain — get four waves per front: whole levels from the
        // top down while a level has at most GS_BLOCK_FRONTS (512) fronts (those workgroups are all resident at once)
        { const int thr = opt.block_fronts;
          int nb = 0;
          const int lowest = S.sub_n > 0 ? 2 : (S.leaf_n > 0 ? 1 : 0);      // the first level of the flagged launch
          for (int l = nlev - 1; l >= lowest; --l) { const int nl = ls.start[l + 1] - ls.start[l];
              if (nl > thr) break;
              nb += nl; }
          S.block_n = std::min(nb, ls.start[nlev] - (S.sub_n > 0 ? S.sub_first + S.sub_n : S.leaf_n)); }
        // the whole-tree backward solve: which levels the flagged launch takes (walk_backsolve_levels)
        { const int wide = opt.bs_wide;
          int l0 = 0;
          if (S.leaf_n != 0) while (l0 + 1 < nlev && ls.start[l0 + 1] - ls.start[l0] > wide) ++l0;
          if (l0 == 0 && nlev > 1 && S.leaf_n != 0) l0 = 1;
          S.bs_l0 = l0;
          // ... and the one light launch below it: the LDS slot of a wave front is ((f + 1) | 1) * npiv doubles, even (launch_backsolve_level)
          auto slot_of = [](int f, int npiv) { return ((((f + 1) | 1) * npiv) + 1) & ~1; };
          S.bs_low = l0 > 0 ? opt.bs_low : 0;
          if (S.bs_low != 0) { int mn = 0, mf = 0;
              for (int l = 1; l < l0; ++l) { mn = std::max(mn, ls.max_npiv[l]); mf = std::max(mf, ls.max_f[l]); }
              S.low_slot = slot_of(ls.max_npiv[0] + ls.max_nbnd[0], ls.max_npiv[0]); S.low_up_slot = slot_of(mf, mn); S.low_n_up = ls.start[l0] - ls.start[1];
              S.low_up_fronts = S.low_n_up > 0 ? std::min(4, std::max(1, 4 * S.low_slot / std::max(S.low_up_slot, 1))) : 4;
              S.low_lds = (size_t)std::max(4 * S.low_slot, S.low_n_up > 0 ? S.low_up_fronts * S.low_up_slot : 0) * sizeof(double); } }
    }
    if (S.big) build_big_tables(P, S);
    return S;
}

// ---- the record of gs_debug_schedule_export: the same walk that gs_solve.cpp launches from, with a sink that writes the launches down
namespace {
enum { L_FACTOR_TREE = 1, L_FACTOR_LEAF, L_FACTOR_LEVEL, L_FACTOR_TOP, L_FACTOR_TAB, L_BACKSOLVE_TREE, L_BACKSOLVE_LEVEL, L_BACKSOLVE_TAB };
struct Recorder {
    const Schedule &S; std::vector<int32_t> &out; int n = 0;
    void rec(int kind, int first, int count, size_t lds, int cls, int table) {
        if (count <= 0) return;                                      // (the launchers return at once: no launch)
        const int32_t r[6] = {kind, first, count, (int32_t)lds, cls, table}; out.insert(out.end(), r, r + 6); ++n; }
    void epoch() {}
    void factor_tree(int n_leaf, int, int, int count, int, int, int n_sub) {
        if (count == n_leaf) rec(L_FACTOR_LEAF, 0, count, 0, 0, -1);       // the leaf instance alone
        else rec(L_FACTOR_TREE, 0, count, n_sub > 0 ? factor_sub_lds_bytes(S.leaf_slot) : 0, 0, -1); }
    void factor_level(int off, int count, int, int mode) { rec(L_FACTOR_LEVEL, off, count, 0, mode, -1); }
    void factor_tree_top(int first, int count) { rec(L_FACTOR_TOP, first, count, 0, 2, -1); }
    void factor_tab(int t, int first, int n_wg, int, size_t lds, int cls, int) { rec(L_FACTOR_TAB, first, n_wg, lds, cls, t); }
    void backsolve_tree(int first, int count, int, int) { rec(L_BACKSOLVE_TREE, first, count, 0, 0, -1); }
    void backsolve_low(int first, int count, int, int, int, int, size_t lds) { rec(L_BACKSOLVE_TREE, first, count, lds, 0, -1); }     // the flagged kind: its fronts order themselves
    void backsolve_level(int off, int count, int, int) { rec(L_BACKSOLVE_LEVEL, off, count, 0, 0, -1); }
    void backsolve_tab(int t, int first, int n_wg, int, int, size_t lds, int cls) { rec(L_BACKSOLVE_TAB, first, n_wg, lds, cls, t); }
};
}  // namespace

void export_schedule(const Plan &P, const Schedule &S, std::vector<int32_t> &out) {
    out.clear();
    const int nlev = (int)S.own.start.size() - 1, n_own = (int)P.level_fronts_owned.size(), n_shared = (int)P.level_fronts_shared.size();
    const int32_t hdr[20] = {0x47535331, std::max(nlev, 0), n_own, n_shared, S.shared_base, S.factor_variant, S.big ? 1 : 0,
                             S.leaf_n, S.leaf_slot, S.leaf_max_f, S.sub_n, S.sub_first, S.sub_free, S.block_n, S.bs_l0,
                             S.small_max_npiv, S.small_max_f, 0, 0, 0};
    out.insert(out.end(), hdr, hdr + 20);
    auto app = [&](const std::vector<int32_t> &v) { out.insert(out.end(), v.begin(), v.end()); };
    app(S.own.start); app(S.shared.start); app(P.level_fronts_owned); app(P.level_fronts_shared);
    for (const WgTable &t : S.tab) { out.push_back((int32_t)t.wg.size() / 2); app(t.wg); }
    for (int tree = 1; tree >= 0; --tree) {
        const size_t at = out.size(); out.push_back(0);
        Recorder R{S, out};
        walk_local(S, tree != 0, R); walk_finish_factor(S, tree != 0, R); walk_finish_backsolve(S, tree != 0, R);
        out[at] = R.n; }
}

}  // namespace gs
