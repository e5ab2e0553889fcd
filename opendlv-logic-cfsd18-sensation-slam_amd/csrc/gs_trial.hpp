// gs_trial.hpp — what the step-control methods (gs_optimize_lm, gs_optimize_dogleg) share on the host: the leading part of their device
// records, the handle's workspace, and the carving of its one device allocation.  Plain C++, no HIP include (tests/trial_layout_san.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

namespace gs {

// The leading part of LmState / DlState: what the host's trial loop and the shared half of the verdict (gs_trial_dev.hpp) read and write
struct TrialState {
    double chi_old;             // chi2 at the accepted point the trial started from (filed behind the update, trial_file)
    double chi_base;            // chi2 at the last accepted point
    int32_t iterations, trials, rejected, terminated;       // accepted iterations, trials, rejected trials, "terminate"
    int32_t done;               // budget used up or terminated: every later enqueued trial is a no-op
    int32_t trials_iter;        // rejected trials of the current iteration
    int32_t failcode;           // d.fail[0] as trial_file found it
    int32_t budget, max_trials, pad;
};
// The leading part of LmDev / DlDev: everything but the method's own record and history
struct TrialDev {
    double *hist_chi2 = nullptr; int32_t *hist_trials = nullptr;    // [64] per ITERATION: chi2 at its starting point, trials it took
    double *base_pose = nullptr, *base_cs = nullptr, *base_lm = nullptr;   // the accepted estimates: [3 NP], [2 NP], [2 ML]  (NP = N + tN, ML = M + tM)
    double *part = nullptr; int32_t n_part = 0;                     // one partial per workgroup of the vertex-parallel kernels
};
// A method's workspace on the handle: one allocation of its own (not pool memory: it outlives the plans), grow-only, sized for cap_p
// poses / cap_l landmarks (tail included); host[0] is the record a call starts from, host[1] the last one read back
template <class Dev, class State> struct TrialWs { Dev dev{}; void *mem = nullptr; size_t cap_p = 0, cap_l = 0; State host[2]{}; };
// What a method keeps in the allocation besides the common arrays: its double-buffered record, further [64] history arrays (at most 2
// of a type), partial arrays of cpart doubles, vertex-order vectors in pairs of [3 cp] and [2 cl] doubles (at most 4 pairs)
struct TrialExtras { size_t state_bytes; int hist_f64, hist_i32, part_arrays, vec_pairs; };
// capacities (poses, landmarks, workgroups), the offset of every array, the size of the allocation
struct TrialLayout { size_t cp, cl, cpart, state, hist_chi2, hist_f64[2], hist_trials, hist_i32[2], base_pose, base_cs, base_lm, part, vec_pose[4], vec_lm[4], total; };
// every block starts on a multiple of 256 bytes; the capacities leave 64 vertices of slack
inline TrialLayout trial_carve(size_t NP, size_t ML, const TrialExtras &x) {
    TrialLayout L{};
    L.cp = NP + 64; L.cl = ML + 64; L.cpart = (L.cp + L.cl + 255) / 256 + 1;
    auto take = [&L](size_t b) { const size_t o = L.total; L.total += (b + 255) & ~(size_t)255; return o; };
    L.state = take(x.state_bytes); L.hist_chi2 = take(64 * 8);
    for (int k = 0; k < x.hist_f64; ++k) L.hist_f64[k] = take(64 * 8);
    L.hist_trials = take(64 * 4);
    for (int k = 0; k < x.hist_i32; ++k) L.hist_i32[k] = take(64 * 4);
    L.base_pose = take(L.cp * 24); L.base_cs = take(L.cp * 16); L.base_lm = take(L.cl * 16); L.part = take((size_t)x.part_arrays * L.cpart * 8);
    for (int k = 0; k < x.vec_pairs; ++k) { L.vec_pose[k] = take(L.cp * 24); L.vec_lm[k] = take(L.cl * 16); }
    return L;
}

}  // namespace gs
