// gs_schedule.hpp — the solver launches of one iteration as a function of the plan and the options (host only: no device call).
// build_schedule decides everything once, with the plan; walk_* turn a Schedule and a launch mode (whole-tree launches, or one
// launch per level after a flag timeout) into the sequence of launches, handed to a sink: gs_solve.cpp's sink launches them,
// export_schedule's records them (gs_debug_schedule_export).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/graphslam_debug.h"
#include "gs_host.hpp"

namespace gs {

// launch parameters of one list of fronts grouped by level
struct LevelSet { std::vector<int32_t> start; std::vector<int> max_f, max_npiv, max_nbnd; };
// a run of table entries of one level with the same LDS need and kernel class
struct WgSeg { int first, count, level; size_t lds; int cls; };
// plans that hold a front of more than 63 scalars: table-driven launches (workgroup -> {level position, kind | count << 8})
struct WgTable { std::vector<int32_t> wg; std::vector<WgSeg> seg; };
enum { TAB_F = 0, TAB_B, TAB_SC, TAB_ST, TAB_SB, N_TABS };     // own factor / backward solve; the SHARED top of a sharded plan: contributions, top, backward solve

struct Schedule {
    int factor_variant = 0;                 // device-side code: 3 = matrix-core LDL^T fronts, 0 = block-per-front (the C-ABI's variant 4)
    bool big = false;                       // variant 3 and a front of more than 63 scalars: the tables below drive the launches
    LevelSet own, shared;                   // this rank's fronts / the shared top (pose-window shards)
    int shared_base = 0;                    // offset of the shared list inside the device's level list
    int64_t front_ws_stride = 0, ws_blocks = 0;     // fronts beyond the LDS limit: doubles per workspace slice, slices
    // decided when variant 3 runs whole-tree launches (gs_debug_options.tree != 0) over at least one own level; else none (all zero)
    int leaf_n = 0, leaf_slot = 0, leaf_max_f = 0;  // level-0 fronts handled by the leaf instance of the factor kernel, its LDS slot (doubles per wave), largest leaf front (<= 47: the three-tile-row leaf instance)
    int sub_n = 0, sub_first = 0, sub_free = 0;     // bottom subtrees (k_factor3_sub): level-1 fronts [sub_first, sub_first + sub_n) each take the leaves below them; the leaf launch covers [0, sub_free)
    int block_n = 0;                        // trailing level positions of the whole-tree factor launch that get a workgroup each
    int bs_l0 = 0;                          // whole-tree backward solve: levels >= bs_l0 in the flagged launch, the wide levels below in one light polling launch (bs_low) or one light launch each
    // the light polling launch over levels bs_l0 - 1 .. 0 (gs_debug_options.bs_low; 0: off): LDS slots of the leaves (low_slot doubles, four
    // to a workgroup) and of the low_n_up positions above them (low_up_slot, low_up_fronts to a workgroup: what fits the leaves' LDS, at least one)
    int bs_low = 0, low_n_up = 0, low_up_fronts = 4, low_up_slot = 0, low_slot = 0; size_t low_lds = 0;
    int small_max_npiv = 0, small_max_f = 0;
    WgTable tab[N_TABS];
};

// factor_variant: the device-side code above; tree_wanted: gs_debug_options.tree != 0.  The launch mode a handle is in and its call
// history are no inputs.  pos_of_front: front -> level position (own list, then the shared one); read for variant 3 only.
Schedule build_schedule(const Plan &P, const std::vector<int32_t> &pos_of_front, int factor_variant, bool tree_wanted, const gs_debug_options &opt);
// the flat record gs_debug_schedule_export documents (include/graphslam_debug.h)
void export_schedule(const Plan &P, const Schedule &S, std::vector<int32_t> &out);

// launches = maximal runs of table entries with the same LDS need (whole-tree mode: across levels; after a flag timeout: never
// across a level, so that no workgroup waits for one of its own launch)
template <class Launch> void for_each_run(const std::vector<WgSeg> &segs, bool across_levels, Launch &&fn) {
    for (size_t i = 0; i < segs.size(); ) {
        size_t j = i + 1; int n = segs[i].count;
        while (j < segs.size() && segs[j].lds == segs[i].lds && segs[j].cls == segs[i].cls && (across_levels || segs[j].level == segs[i].level)) { n += segs[j].count; ++j; }
        fn(segs[i].first, n, segs[i].lds, segs[i].cls);
        i = j; }
}
// A sink has one member per launcher of gs_device.hpp that the solver phases use (same arguments without the device state and
// the stream; a table launch names its table by TAB_*), and epoch(): a new generation of completion flags.
// the shared top of a sharded plan with workgroup fronts: contributions (mode 1), the top from the exchange (mode 2), its backward solve
template <class Sink> void walk_shared_big(const Schedule &S, bool tree, int what, Sink &sink) {
    if (what == 1) for_each_run(S.tab[TAB_SC].seg, true, [&](int first, int n, size_t lds, int cls) { sink.factor_tab(TAB_SC, first, n, 0, lds, cls, 1); });
    else if (what == 2) for_each_run(S.tab[TAB_ST].seg, tree, [&](int first, int n, size_t lds, int cls) { sink.factor_tab(TAB_ST, first, n, 0, lds, cls, 2); });
    else for_each_run(S.tab[TAB_SB].seg, tree, [&](int first, int n, size_t lds, int cls) { sink.backsolve_tab(TAB_SB, first, n, S.small_max_npiv, S.small_max_f, lds, cls); });
}
template <class Sink> void walk_factor_big(const Schedule &S, const LevelSet &ls, bool tree, Sink &sink) {
    if (S.leaf_n > 0) sink.factor_tree(S.leaf_n, S.leaf_slot, S.leaf_max_f, S.leaf_n, 0, 0, 0);       // the leaf instance alone
    // "no flags to wait for at level 1" holds only if EVERY leaf went through the leaf launch (big leaves share the table launch with their parents)
    const int leaf_pre = (S.leaf_n > 0 && S.leaf_n == ls.start[1]) ? 1 : 0;
    for_each_run(S.tab[TAB_F].seg, tree, [&](int first, int n, size_t lds, int cls) { sink.factor_tab(TAB_F, first, n, leaf_pre, lds, cls, 0); });
}
// own fronts bottom-up (mode 0), shared top bottom-up from the all-reduced exchange buffer (mode 2)
template <class Sink> void walk_factor_levels(const Schedule &S, bool tree, const LevelSet &ls, int base, int mode, Sink &sink) {
    const int nlev = (int)ls.start.size() - 1; const bool v3 = S.factor_variant == 3;
    if (v3 && tree && mode == 0 && base == 0 && nlev > 0) {     // every own level in one launch
        sink.epoch();
        if (S.big) { walk_factor_big(S, ls, true, sink); return; }
        sink.factor_tree(S.sub_n > 0 ? S.sub_free : S.leaf_n, S.leaf_slot, S.leaf_max_f, ls.start[nlev], S.block_n, S.sub_first, S.sub_n); return; }
    if (S.big && !tree && mode == 0 && base == 0 && nlev > 0) { sink.epoch(); walk_factor_big(S, ls, false, sink); return; }
    if (S.big && mode == 2 && nlev > 0 && ls.start[nlev] > 0) { walk_shared_big(S, tree, 2, sink); return; }     // ... of a plan with workgroup fronts: table-driven
    if (v3 && tree && mode == 2 && nlev > 0 && ls.start[nlev] > 0) {     // the shared top of a sharded graph, one flagged launch
        sink.factor_tree_top(base, ls.start[nlev]); return; }
    for (int l = 0; l < nlev; ++l)
        sink.factor_level(base + ls.start[l], ls.start[l + 1] - ls.start[l], ls.max_f[l], mode);
}
template <class Sink> void walk_backsolve_levels(const Schedule &S, bool tree, const LevelSet &ls, int base, Sink &sink) {
    const int nlev = (int)ls.start.size() - 1; const bool v3 = S.factor_variant == 3;
    if (S.big && base == 0 && nlev > 0) {
        for_each_run(S.tab[TAB_B].seg, tree, [&](int first, int n, size_t lds, int cls) { sink.backsolve_tab(TAB_B, first, n, S.small_max_npiv, S.small_max_f, lds, cls); });
        return; }
    if (S.big && base != 0 && nlev > 0 && ls.start[nlev] > 0) { walk_shared_big(S, tree, 3, sink); return; }
    if (v3 && tree && base == 0 && nlev > 0) {
        // levels >= 1 in one launch (fronts wait for their parent's flag), then the leaf level on its own: by then every
        // parent is done, so it needs no flags, and its LDS slot is sized for the leaves alone (more resident waves)
        // The flagged launch is register-heavy (each lane preloads its L columns: 2 waves per SIMD) — right for the chain
        // of the upper levels (2.2 us per level), wrong for the wide levels at the bottom, which are bound by resident
        // waves x bytes: levels of more than GS_BS_WIDE (1024) fronts leave it for the light path, like the leaves
        // (measured per-level completion times: scripts/level_times.py).  Those wide levels share ONE launch (bs_low): its fronts
        // poll their boundary rows like the flagged launch's, so the levels need no boundary between them and the leaves' panels
        // stream while the level above still computes; bs_low = 0 keeps a launch per level.
        const int l0 = S.bs_l0;
        int mn = 0, mf = 0; for (int l = l0; l < nlev; ++l) { mn = std::max(mn, ls.max_npiv[l]); mf = std::max(mf, ls.max_f[l]); }
        sink.backsolve_tree(ls.start[l0], ls.start[nlev] - ls.start[l0], mn, mf);
        if (S.bs_low != 0 && l0 > 0) { sink.backsolve_low(0, ls.start[l0], S.low_n_up, S.low_up_fronts, S.low_up_slot, S.low_slot, S.low_lds); return; }
        for (int l = l0 - 1; l >= 0; --l) sink.backsolve_level(ls.start[l], ls.start[l + 1] - ls.start[l], ls.max_npiv[l], ls.max_nbnd[l]);
        return; }
    if (v3 && tree && base != 0 && nlev > 0 && ls.start[nlev] > 0) {      // shared top: one flagged launch, root first
        int mn = 0, mf = 0; for (int l = 0; l < nlev; ++l) { mn = std::max(mn, ls.max_npiv[l]); mf = std::max(mf, ls.max_f[l]); }
        sink.backsolve_tree(base, ls.start[nlev], mn, mf); return; }
    for (int l = nlev - 1; l >= 0; --l)
        sink.backsolve_level(base + ls.start[l], ls.start[l + 1] - ls.start[l], ls.max_npiv[l], ls.max_nbnd[l]);
}
// the solver launches of one iteration, in order.  First half of a pose-window shard: its own subtrees, then its contribution to
// every shared front into the exchange buffer; second half: the shared top (redundantly on every rank), backward solve top-down
template <class Sink> void walk_local(const Schedule &S, bool tree, Sink &sink) {
    walk_factor_levels(S, tree, S.own, 0, 0, sink);
    const int nshared = S.shared.start.empty() ? 0 : S.shared.start.back();
    if (nshared > 0 && S.big) walk_shared_big(S, tree, 1, sink);      // a plan with workgroup fronts: table-driven
    else if (nshared > 0) { int mf = 0; for (int v : S.shared.max_f) mf = std::max(mf, v);
        sink.factor_level(S.shared_base, nshared, mf, 1); }
}
template <class Sink> void walk_finish_factor(const Schedule &S, bool tree, Sink &sink) { walk_factor_levels(S, tree, S.shared, S.shared_base, 2, sink); }
template <class Sink> void walk_finish_backsolve(const Schedule &S, bool tree, Sink &sink) {
    walk_backsolve_levels(S, tree, S.shared, S.shared_base, sink);
    walk_backsolve_levels(S, tree, S.own, 0, sink);
}

}  // namespace gs
