// gs_layout.hpp — the plain-data formats that the upload (gs_upload.cpp) writes and the structure-phase kernels (gs_kernels.hip) read:
// the device mirror of a front, the parts of the one arena that holds block-sparse H and b, the argument record of k_build_sc3 and the
// slots of a growth patch record.  No HIP in here: tests/upload_tables_san.cpp compiles it with the host sanitizers.
#pragma once
#include <cstdint>

namespace gs {

// Mirror of Front for the device (POD, 80 bytes)
struct DevFront {
    int32_t npiv, nbnd, piv0, parent;
    int32_t asm_off, asm_cnt, asm_dup, child_off;
    int32_t child_cnt, owner, level, pad0;
    int64_t bnd_off, map_off, L_off, U_off;
};

// H_arena, part by part in this order.  The last six are the blocks of a grown plan's tail (grow_plan): diagonal blocks and rhs of
// the tail poses / landmarks, off-diagonal blocks of the tail edges.
enum ArenaPart : int { ARENA_Hpp_diag, ARENA_b_pose, ARENA_Hpp_off, ARENA_Hpl, ARENA_lm_part, ARENA_Hll_diag, ARENA_b_lm,
                       ARENA_t_Hpp_diag, ARENA_t_b_pose, ARENA_t_Hpp_off, ARENA_t_Hpl, ARENA_t_Hll_diag, ARENA_t_b_lm, ARENA_PARTS };
constexpr int ARENA_TAIL = ARENA_t_Hpp_diag;                    // the first tail part: Sc3Args::toff[part - ARENA_TAIL]
constexpr int LM_REC = 8;       // doubles per (wave tile, landmark) partial-sum record of lm_part: {H00, H01, H11, b0, b1, -, -, -} = one 64-byte line
struct ArenaCounts { int64_t N, Epp, ell_len, n_groups, M, tcapN, tcapEpp, tcapEpl, tcapM; };     // base counts, then the tail capacities
struct ArenaOffsets { int64_t at[ARENA_PARTS + 1];             // in doubles; at[ARENA_PARTS] = the whole arena
                      int64_t doubles() const { return at[ARENA_PARTS]; } };
// Every part starts 16-byte aligned (the fused linearisation kernel stores Hpp_diag's 6 planes and b_pose's 3 as 9 contiguous planes:
// 6 N is even, no padding between), the partial-sum records of lm_part on a 64-byte line.  false: beyond the 32-bit offsets the
// front assembly names every scalar by.
inline bool arena_layout(const ArenaCounts &c, ArenaOffsets &o) {
    const int64_t sizes[ARENA_PARTS] = {c.N * 6, c.N * 3, c.Epp * 9, c.ell_len * 6, c.n_groups * LM_REC, c.M * 3, c.M * 2,
                                        c.tcapN * 6, c.tcapN * 3, c.tcapEpp * 9, c.tcapEpl * 6, c.tcapM * 3, c.tcapM * 2};
    o.at[0] = 0;
    for (int k = 0; k < ARENA_PARTS; ++k) { o.at[k + 1] = o.at[k] + ((sizes[k] + 1) & ~(int64_t)1);
        if (k + 1 == ARENA_lm_part) o.at[k + 1] = (o.at[k + 1] + 7) & ~(int64_t)7; }
    return o.doubles() < ((int64_t)1 << 31);
}

// structure phase on the device: expand the block assembly records into scalar / landmark records (k_build_sc3)
struct Sc3Args { int64_t off[8]; int64_t L; int32_t N, M, Epp, fused;         // off[ArenaPart] of the base parts (and of the first tail part)
                 int64_t toff[6]; int32_t tcapN, tcapEpp, tcapEpl, tcapM; };   // tail blocks: toff[ArenaPart - ARENA_TAIL]; plane strides
inline Sc3Args sc3_args(const ArenaOffsets &o, const ArenaCounts &c, bool fused) {
    Sc3Args A;
    for (int k = 0; k < 8; ++k) A.off[k] = o.at[k];
    A.L = c.ell_len; A.N = (int32_t)c.N; A.M = (int32_t)c.M; A.Epp = (int32_t)c.Epp; A.fused = fused ? 1 : 0;
    for (int k = 0; k < 6; ++k) A.toff[k] = o.at[ARENA_TAIL + k];
    A.tcapN = (int32_t)c.tcapN; A.tcapEpp = (int32_t)c.tcapEpp; A.tcapEpl = (int32_t)c.tcapEpl; A.tcapM = (int32_t)c.tcapM;
    return A;
}

// growth: one patch record per changed front (k_apply_front_patch scatters it into fronts / u3_off / u3_size / bf)
enum PatchSlot : int { PATCH_FRONT = 0, PATCH_DEVFRONT = 1 /* 20 ints */, PATCH_U3_OFF = 21, PATCH_U3_SIZE = 22, PATCH_BF = 23 /* 8 ints */,
                       PATCH_SPARE = 31, PATCH_INTS = 32 };
static_assert(sizeof(DevFront) == 4 * (PATCH_U3_OFF - PATCH_DEVFRONT), "DevFront travels as 20 ints");

}  // namespace gs
