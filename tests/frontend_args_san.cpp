// frontend_args_san.cpp — a stand-alone program (its own main) linked with the library's host objects built under AddressSanitizer and
// UndefinedBehaviorSanitizer (`make -C csrc frontend_args_san` builds and runs it).  On a host-only handle it drives the argument checks of the
// front end's batch and resident entry points — the paths that run before a call builds its observation and map views: null pointers, bad
// frame bounds, pose indices out of range, a wrong struct_size, a frame above GS_NN_FRAME_MAX, a misaligned dev_obs — and, with everything
// in order, the refusal of the host-only handle.  Every one of these returns before the first device call, so no GPU is needed; the
// "device" pointers of the resident calls are host memory that is never read.
#include "graphslam.h"

#include <cstdio>
#include <cstring>
#include <vector>

static int fails = 0;
// the call is refused with `code`, and the message names the reason
static void refused(int rc, int code, const char *needle, const char *what) {
    const char *msg = gs_last_error();
    if (rc == code && msg && std::strstr(msg, needle)) return;
    std::printf("FAIL %s: rc %d (want %d), message \"%s\" (want \"%s\")\n", what, rc, code, msg ? msg : "", needle);
    ++fails;
}
#define REFUSED(call, needle) refused((call), GS_ERR_INVALID, needle, #call)
#define NO_DEVICE(call) refused((call), GS_ERR_NO_DEVICE, "", #call)

int main() {
    gs_config cfg; gs_config_default(&cfg); cfg.device = -2;
    gs_graph *g = nullptr;
    if (gs_create(&cfg, &g) != GS_OK || !g) { std::printf("FAIL gs_create (host-only): %s\n", gs_last_error()); return 1; }
    const int n = 5, npose = 2, n_map = 3, nf = 2;
    alignas(32) double obs[4 * n] = {}; double poses[3 * npose] = {}, map_xy[2 * n_map] = {}, az[n] = {}, out2[2 * n] = {}, d2[n] = {}, sec[n] = {};
    double pose3[3 * nf] = {}, cov9[9 * nf] = {}, chi2[nf] = {}, cost[nf] = {}, e2[n] = {};
    int32_t pose_of[n] = {0, 0, 0, 1, 1}, bad_pose_of[n] = {0, 0, 2, 1, 1}, map_type[n_map] = {1, 2, 3}, fs[nf + 1] = {0, 3, 5}, in_idx[n] = {0, 1, 2, -1, 0};
    int32_t fs_end[nf + 1] = {0, 3, 4}, fs_desc[nf + 1] = {0, 6, 5}, fs_one[2] = {0, n}, idx[n] = {}, na[n] = {}, cnt[nf] = {}, seed[4 * nf] = {}, st[nf] = {};
    int64_t n_seeds[nf] = {};
    gs_nn_params nn; gs_nn_params_default(&nn); gs_nn_params nn_size = nn; nn_size.struct_size -= 4;
    gs_jc_params jc; gs_jc_params_default(&jc); gs_jc_params jc_size = jc; jc_size.struct_size += 8;
    gs_loc_params lo; gs_loc_params_default(&lo); gs_loc_params lo_size = lo; lo_size.struct_size = 0;
    gs_reloc_params rl; gs_reloc_params_default(&rl); gs_reloc_params rl_size = rl; rl_size.struct_size += 1;
    gs_follow_params fo; gs_follow_params_default(&fo); gs_follow_params fo_size = fo; fo_size.struct_size -= 1;

    // ---- the conversions and the Euclidean association
    REFUSED(gs_polar_to_xy_batch(g, n, az, nullptr, az, out2), "bad argument");
    REFUSED(gs_cone_to_global_batch(g, n, poses, npose, bad_pose_of, obs, out2), "pose_of_obs out of range");
    REFUSED(gs_associate_batch(g, n, poses, npose, pose_of, obs, n_map, nullptr, map_type, 1.2, 1e-4, idx), "bad argument");
    REFUSED(gs_associate_batch(g, n, poses, npose, bad_pose_of, obs, n_map, map_xy, map_type, 1.2, 1e-4, idx), "pose_of_obs out of range");
    NO_DEVICE(gs_associate_batch(g, n, poses, npose, pose_of, obs, n_map, map_xy, map_type, 1.2, 1e-4, idx));
    REFUSED(gs_associate_resident(g, n, poses, npose, nullptr, obs, 1.2, 1e-4, idx), "bad argument");
    // ---- covariance-gated association
    REFUSED(gs_associate_nn_batch(g, n, nullptr, npose, pose_of, obs, n_map, map_xy, map_type, nullptr, nullptr, &nn, idx, d2, sec), "bad argument");
    REFUSED(gs_associate_nn_batch(g, n, poses, npose, pose_of, obs, n_map, map_xy, map_type, nullptr, nullptr, &nn_size, idx, d2, sec), "wrong struct_size");
    REFUSED(gs_associate_nn_batch(g, n, poses, npose, bad_pose_of, obs, n_map, map_xy, map_type, nullptr, nullptr, &nn, idx, d2, sec), "pose_of_obs out of range");
    NO_DEVICE(gs_associate_nn_batch(g, n, poses, npose, pose_of, obs, n_map, map_xy, map_type, nullptr, nullptr, &nn, idx, nullptr, nullptr));
    REFUSED(gs_associate_nn_resident(g, n, poses, npose, pose_of, obs, nullptr, nullptr, idx, d2, sec), "null params");
    REFUSED(gs_associate_nn_resident(g, n, poses, npose, pose_of, obs + 1, nullptr, &nn, idx, d2, sec), "32-byte aligned");
    NO_DEVICE(gs_associate_nn_resident(g, n, poses, npose, pose_of, obs, nullptr, &nn, idx, d2, sec));
    // ---- the assignment over frames
    REFUSED(gs_assign_opt_batch(g, n, poses, npose, pose_of, obs, nf, nullptr, n_map, map_xy, map_type, nullptr, nullptr, &nn, idx, d2, na), "bad argument");
    REFUSED(gs_assign_opt_batch(g, n, poses, npose, pose_of, obs, nf, fs_end, n_map, map_xy, map_type, nullptr, nullptr, &nn, idx, d2, na), "begin at 0 and end at n");
    REFUSED(gs_assign_opt_batch(g, n, poses, npose, pose_of, obs, nf, fs_desc, n_map, map_xy, map_type, nullptr, nullptr, &nn, idx, d2, na), "must ascend");
    REFUSED(gs_assign_opt_batch(g, n, poses, npose, bad_pose_of, obs, nf, fs, n_map, map_xy, map_type, nullptr, nullptr, &nn, idx, d2, na), "pose_of_obs out of range");
    REFUSED(gs_assign_nn_batch(g, n, poses, npose, pose_of, obs, nf, fs, n_map, map_xy, map_type, nullptr, nullptr, &nn_size, idx, d2), "wrong struct_size");
    NO_DEVICE(gs_assign_opt_batch(g, n, poses, npose, pose_of, obs, nf, fs, n_map, map_xy, map_type, nullptr, nullptr, &nn, idx, d2, na));
    REFUSED(gs_assign_opt_resident(g, n, poses, npose, pose_of, obs, nf, nullptr, nullptr, &nn, idx, d2, na), "bad argument");
    REFUSED(gs_assign_opt_resident(g, n, poses, npose, pose_of, obs + 2, nf, fs, nullptr, &nn, idx, d2, na), "32-byte aligned");
    {   // a frame of GS_NN_FRAME_MAX + 1 observations: refused by the batch call and by the live call
        const int big = GS_NN_FRAME_MAX + 1;
        std::vector<double> ob(4 * (size_t)big, 1.0), o2(2 * (size_t)big), od(big); std::vector<int32_t> po(big, 0), oi(big), ona(big);
        const int32_t fsb[2] = {0, big};
        REFUSED(gs_assign_opt_batch(g, big, poses, npose, po.data(), ob.data(), 1, fsb, n_map, map_xy, map_type, nullptr, nullptr, &nn, oi.data(), od.data(), ona.data()),
                "more than GS_NN_FRAME_MAX");
        REFUSED(gs_frame_frontend_assign(g, poses, nullptr, ob.data(), big, &nn, o2.data(), o2.data(), oi.data(), od.data()), "more than GS_NN_FRAME_MAX");
        REFUSED(gs_frame_frontend_follow(g, nullptr, nullptr, ob.data(), big, &nn, &jc, &lo, &fo, nullptr, nullptr, nullptr, nullptr), "more than GS_NN_FRAME_MAX");
        REFUSED(gs_relocalize_batch(g, big, ob.data(), 1, fsb, n_map, map_xy, map_type, &rl, pose3, cnt, cost, seed, nullptr, nullptr, n_seeds, st, oi.data(), od.data()),
                "more than GS_NN_FRAME_MAX");
    }
    // ---- joint compatibility and localisation: a hypothesis, one pose per frame
    REFUSED(gs_joint_compat_batch(g, n, poses, npose, pose_of, obs, nf, fs, n_map, map_xy, nullptr, nullptr, &nn, &jc, nullptr, idx, chi2, cnt, cnt, cnt, pose3), "bad argument");
    REFUSED(gs_joint_compat_batch(g, n, poses, npose, pose_of, obs, nf, fs, n_map, map_xy, nullptr, nullptr, &nn, &jc_size, in_idx, idx, chi2, cnt, cnt, cnt, pose3), "wrong struct_size");
    REFUSED(gs_joint_compat_batch(g, n, poses, npose, pose_of, obs, 1, fs_one, n_map, map_xy, nullptr, nullptr, &nn, &jc, in_idx, idx, chi2, cnt, cnt, cnt, pose3), "share one pose");
    in_idx[3] = n_map;
    REFUSED(gs_joint_compat_batch(g, n, poses, npose, pose_of, obs, nf, fs, n_map, map_xy, nullptr, nullptr, &nn, &jc, in_idx, idx, chi2, cnt, cnt, cnt, pose3), "in_index outside");
    REFUSED(gs_localize_batch(g, n, poses, npose, pose_of, obs, nf, fs, n_map, map_xy, nullptr, nullptr, &nn, &lo, in_idx, pose3, cov9, chi2, cnt, cnt, st), "in_index outside");
    in_idx[3] = -1;
    REFUSED(gs_localize_batch(g, n, poses, npose, pose_of, obs, nf, fs, n_map, map_xy, nullptr, nullptr, &nn, &lo_size, in_idx, pose3, cov9, chi2, cnt, cnt, st), "wrong struct_size");
    NO_DEVICE(gs_joint_compat_batch(g, n, poses, npose, pose_of, obs, nf, fs, n_map, map_xy, nullptr, nullptr, &nn, &jc, in_idx, idx, chi2, cnt, cnt, cnt, pose3));
    NO_DEVICE(gs_localize_batch(g, n, poses, npose, pose_of, obs, nf, fs, n_map, map_xy, nullptr, nullptr, &nn, &lo, in_idx, pose3, cov9, chi2, cnt, cnt, st));
    REFUSED(gs_joint_compat_resident(g, n, poses, npose, pose_of, obs, nf, fs, nullptr, &nn, &jc, nullptr, idx, chi2, cnt, cnt, cnt, pose3), "bad argument");
    REFUSED(gs_localize_resident(g, n, poses, npose, pose_of, obs + 3, nf, fs, nullptr, &nn, &lo, in_idx, pose3, cov9, chi2, cnt, cnt, st), "32-byte aligned");
    NO_DEVICE(gs_localize_resident(g, n, poses, npose, pose_of, obs, nf, fs, nullptr, &nn, &lo, in_idx, pose3, cov9, chi2, cnt, cnt, st));
    // ---- relocalisation: no poses
    REFUSED(gs_relocalize_batch(g, n, nullptr, nf, fs, n_map, map_xy, map_type, &rl, pose3, cnt, cost, seed, nullptr, nullptr, n_seeds, st, idx, e2), "bad argument");
    REFUSED(gs_relocalize_batch(g, n, obs, nf, fs, n_map, map_xy, map_type, &rl_size, pose3, cnt, cost, seed, nullptr, nullptr, n_seeds, st, idx, e2), "wrong struct_size");
    REFUSED(gs_relocalize_batch(g, n, obs, nf, fs_end, n_map, map_xy, map_type, &rl, pose3, cnt, cost, seed, nullptr, nullptr, n_seeds, st, idx, e2), "begin at 0 and end at n");
    NO_DEVICE(gs_relocalize_batch(g, n, obs, nf, fs, n_map, map_xy, map_type, &rl, pose3, cnt, cost, seed, cnt, pose3, n_seeds, st, idx, e2));
    REFUSED(gs_relocalize_resident(g, n, obs, nf, nullptr, &rl, pose3, cnt, cost, seed, nullptr, nullptr, n_seeds, st, idx, e2), "bad argument");
    NO_DEVICE(gs_relocalize_resident(g, n, obs, nf, fs, &rl, pose3, cnt, cost, seed, nullptr, nullptr, n_seeds, st, idx, e2));
    // ---- frame following
    REFUSED(gs_follow_batch(g, 1, nullptr, nullptr, nf, n, obs, fs, pose3, nullptr, n_map, map_xy, map_type, nullptr, &nn, &jc, &lo, &fo, nullptr, nullptr, nullptr, nullptr, nullptr),
            "bad argument");
    REFUSED(gs_follow_batch(g, 1, poses, nullptr, nf, n, obs, fs, pose3, nullptr, n_map, map_xy, map_type, nullptr, &nn, &jc, &lo, &fo_size, nullptr, nullptr, nullptr, nullptr, nullptr),
            "wrong struct_size");
    REFUSED(gs_follow_batch(g, GS_FOLLOW_HYP_MAX + 1, poses, nullptr, nf, n, obs, fs, pose3, nullptr, n_map, map_xy, map_type, nullptr, &nn, &jc, &lo, &fo, nullptr, nullptr, nullptr,
                            nullptr, nullptr), "n_hyp outside");
    REFUSED(gs_follow_batch(g, 1, poses, nullptr, nf, n, obs, fs_desc, pose3, nullptr, n_map, map_xy, map_type, nullptr, &nn, &jc, &lo, &fo, nullptr, nullptr, nullptr, nullptr, nullptr),
            "must ascend");
    NO_DEVICE(gs_follow_batch(g, 1, poses, nullptr, nf, n, obs, fs, pose3, nullptr, n_map, map_xy, map_type, nullptr, &nn, &jc, &lo, &fo, nullptr, idx, nullptr, nullptr, nullptr));
    REFUSED(gs_follow_resident(g, 1, poses, nullptr, nf, n, obs, fs, GS_NN_FRAME_MAX + 1, pose3, nullptr, &nn, &jc, &lo, &fo, nullptr, nullptr, nullptr, nullptr), "frame_cap outside");
    NO_DEVICE(gs_follow_resident(g, 1, poses, nullptr, nf, n, obs, fs, 4, pose3, nullptr, &nn, &jc, &lo, &fo, nullptr, nullptr, nullptr, nullptr));
    // ---- the resident map
    REFUSED(gs_map_append(g, n_map, nullptr, map_type), "bad argument");
    REFUSED(gs_map_set_xy(g, 0, 1, map_xy), "beyond the end of the map");
    if (gs_map_clear(g) != GS_OK || gs_map_size(g) != 0) { std::printf("FAIL gs_map_clear on the empty map\n"); ++fails; }
    gs_destroy(g);
    if (fails) return 1;
    std::printf("front-end arguments: ok\n");
    return 0;
}
