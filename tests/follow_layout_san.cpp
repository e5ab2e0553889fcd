// follow_layout_san.cpp — a stand-alone program (its own main, no HIP) around csrc/gs_follow_host.hpp, built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_follow_cpu.py.  For every size the following calls can ask for it carves the stage and chain
// buffers out of a heap block of exactly FollowLayout::bytes and writes every piece to its last byte, as the kernels do for n_hyp frames of
// `cap` observations: a piece that overlaps its neighbour, leaves the block or breaks its alignment is found here.  The frame call's staging
// is filled the same way at its largest.
#include "gs_follow_host.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace gs;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static void one(int n_hyp, int cap) {
    FollowLayout L;
    CHECK(follow_layout(n_hyp, cap, L));
    std::vector<unsigned char> mem(L.bytes, 0);
    const size_t nh = (size_t)n_hyp, no = nh * (size_t)cap;
    struct Piece { size_t off, bytes, align; unsigned char tag; };
    const Piece ps[] = {{L.obs, no * 32, 32, 1}, {L.pose_of_obs, no * 4, 4, 2}, {L.frame_start, (nh + 1) * 4, 4, 3}, {L.pose, nh * 24, 8, 4}, {L.cov, nh * 72, 8, 5},
                        {L.as_idx, no * 4, 4, 6}, {L.as_d2, no * 8, 8, 7}, {L.jc_idx, no * 4, 4, 8}, {L.jc_kept, nh * 4, 4, 9}, {L.lo_pose, nh * 24, 8, 10},
                        {L.lo_cov, nh * 72, 8, 11}, {L.lo_chi2, nh * 8, 8, 12}, {L.lo_pairs, nh * 4, 4, 13}, {L.lo_iters, nh * 4, 4, 14}, {L.lo_status, nh * 4, 4, 15}};
    for (const Piece &p : ps) { CHECK(p.off % 256 == 0 && p.off % p.align == 0); CHECK(p.off + p.bytes <= L.bytes);
        if (p.bytes) std::memset(mem.data() + p.off, p.tag, p.bytes); }
    for (const Piece &p : ps)                                                  // nobody wrote into anybody else
        for (size_t b = 0; b < p.bytes; ++b) if (mem[p.off + b] != p.tag) { CHECK(!"a piece was overwritten"); break; }
}

int main() {
    FollowLayout L;
    CHECK(!follow_layout(0, 8, L) && !follow_layout(65, 8, L) && !follow_layout(1, -1, L) && !follow_layout(1, 257, L));
    const int hyps[] = {1, 2, 63, 64}, caps[] = {0, 1, 64, 65, 255, 256};
    for (int h : hyps) for (int c : caps) one(h, c);
    using Io = FollowFrameIo;
    CHECK(Io::IN_OBS % 32 == 0 && Io::IN_COV >= Io::IN_MOTION + 24 && Io::IN_FS >= Io::IN_COV + 72 && Io::IN_OBS >= Io::IN_FS + 8);
    CHECK(Io::in_bytes(FOLLOW_FRAME_MAX) == Io::IN_BYTES && Io::in_bytes(0) == Io::IN_OBS);
    CHECK(Io::OUT_BEST == (size_t)FOLLOW_HYP_MAX * FOLLOW_STEP_BYTES && Io::OUT_IDX >= Io::OUT_BEST + 8 && Io::OUT_IDX % 4 == 0);
    std::vector<unsigned char> in(Io::IN_BYTES), out(Io::OUT_BYTES);
    std::memset(in.data() + Io::IN_OBS, 1, (size_t)FOLLOW_FRAME_MAX * 32);
    std::memset(out.data() + Io::OUT_IDX, 2, (size_t)FOLLOW_HYP_MAX * FOLLOW_FRAME_MAX * 4);
    if (fails == 0) std::printf("follow layout: ok\n");
    return fails ? 1 : 0;
}
