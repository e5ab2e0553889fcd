// frame_layout_san.cpp — a stand-alone program (its own main, no HIP) around csrc/gs_frame_host.hpp, built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_frame_calls_cpu.py.  For every frame size at which the live calls' staging changes its shape it
// carves each of the three input formats, in and out, from heap blocks of exactly the computed sizes and writes every piece to its last byte,
// as the host and the kernels do: a piece that overlaps its neighbour, leaves the block or breaks its alignment is found here.  The record
// structs are held to the byte offsets the kernels' pointers have always had, and written through to their last member.
#include "gs_frame_host.hpp"

#include <cstddef>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

using namespace gs;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

struct Piece { size_t off, bytes, align; };
// the pieces in a block of exactly `total` bytes: aligned, inside, disjoint, and the block has no byte that nobody owns behind the last piece
static void carve(const std::vector<Piece> &ps, size_t total) {
    std::vector<unsigned char> mem(total, 0);
    size_t end = 0; unsigned char tag = 0;
    for (const Piece &p : ps) { ++tag;
        CHECK(p.off != FrameLayout::NONE); CHECK(p.off % p.align == 0); CHECK(p.off + p.bytes <= total);
        if (p.off + p.bytes > total) continue;                                  // (reported; not written)
        if (p.bytes) std::memset(mem.data() + p.off, tag, p.bytes);
        if (p.off + p.bytes > end) end = p.off + p.bytes; }
    CHECK(end == total || ps.empty());
    tag = 0;
    for (const Piece &p : ps) { ++tag;                                          // nobody wrote into anybody else
        if (p.off + p.bytes > total) continue;
        for (size_t b = 0; b < p.bytes; ++b) if (mem[p.off + b] != tag) { CHECK(!"a piece was overwritten"); break; } }
}

static void one(size_t k) {
    FrameLayout L = frame_layout_plain(k);                                      // k_frame_frontend's format: the observations follow the pose (doubles, 8)
    CHECK(L.cov == FrameLayout::NONE && L.frame_start == FrameLayout::NONE && L.pose_of_obs == FrameLayout::NONE && L.d2 == FrameLayout::NONE &&
          L.second == FrameLayout::NONE && L.na == FrameLayout::NONE);
    CHECK(L.obs == 24 && L.in_bytes == 24 + 32 * k && L.out_bytes == 36 * k);
    carve({{L.pose, 24, 8}, {L.obs, 32 * k, 8}}, L.in_bytes);
    carve({{L.z, 16 * k, 8}, {L.g, 16 * k, 8}, {L.idx, 4 * k, 4}}, L.out_bytes);

    L = frame_layout_nn(k);                                                     // k_frame_nn's: one 32-byte load per observation
    CHECK(L.frame_start == FrameLayout::NONE && L.pose_of_obs == FrameLayout::NONE && L.na == FrameLayout::NONE);
    CHECK(L.cov == 24 && L.obs == 96 && L.in_bytes == 96 + 32 * k && L.out_bytes == 52 * k);
    carve({{L.pose, 24, 8}, {L.cov, 72, 8}, {L.obs, 32 * k, 32}}, L.in_bytes);
    carve({{L.z, 16 * k, 8}, {L.g, 16 * k, 8}, {L.d2, 8 * k, 8}, {L.second, 8 * k, 8}, {L.idx, 4 * k, 4}}, L.out_bytes);

    L = frame_layout_chain(k);                                                  // the batch kernels' arrays for one pose and one frame
    CHECK(L.second == FrameLayout::NONE);
    CHECK(L.cov == 32 && L.obs == 128 && L.frame_start == 128 + 32 * k && L.in_bytes == 136 + 36 * k && L.out_bytes == 48 * k);
    CHECK(L.na + 4 * k == L.out_bytes && L.idx + 4 * k == L.na);                // the greedy assignment copies [0, na) back: everything but the counts
    carve({{L.pose, 24, 8}, {L.cov, 72, 8}, {L.obs, 32 * k, 32}, {L.frame_start, 8, 4}, {L.pose_of_obs, 4 * k, 4}}, L.in_bytes);
    carve({{L.z, 16 * k, 8}, {L.g, 16 * k, 8}, {L.d2, 8 * k, 8}, {L.idx, 4 * k, 4}, {L.na, 4 * k, 4}}, L.out_bytes);
}

int main() {
    const size_t ks[] = {0, 1, 64, 65, 255, 256};
    for (size_t k : ks) one(k);
    CHECK(FRAME_MAX == 256);
    // the records: the byte offsets of the device pointers, and every member written in a heap block of exactly the struct's size
    CHECK(offsetof(JcRec, j) == 0 && offsetof(JcRec, delta) == 8 && offsetof(JcRec, kept) == 32 && offsetof(JcRec, dropped) == 36 && offsetof(JcRec, untestable) == 40);
    CHECK(offsetof(JcRec, index) == 48 && sizeof(JcRec) == 48 + 4 * 256);
    CHECK(offsetof(LoRec, pose) == 0 && offsetof(LoRec, cov) == 24 && offsetof(LoRec, chi2) == 96 && offsetof(LoRec, pairs) == 104 && offsetof(LoRec, iterations) == 108);
    CHECK(offsetof(LoRec, status) == 112 && sizeof(LoRec) == 120);
    CHECK(offsetof(ChainRec, jc) == 0 && offsetof(ChainRec, lo) == 1072 && sizeof(ChainRec) == 1192);
    CHECK(offsetof(RelocRec, pose) == 0 && offsetof(RelocRec, second_pose) == 24 && offsetof(RelocRec, cost) == 48 && offsetof(RelocRec, n_seeds) == 56);
    CHECK(offsetof(RelocRec, seed) == 64 && offsetof(RelocRec, count) == 80 && offsetof(RelocRec, second_count) == 84 && offsetof(RelocRec, status) == 88);
    CHECK(offsetof(RelocRec, index) == 96 && offsetof(RelocRec, e2) == 1120 && sizeof(RelocRec) == 1120 + 8 * 256);
    CHECK(alignof(ChainRec) == 8 && alignof(RelocRec) == 8);
    std::vector<unsigned char> cm(sizeof(ChainRec)), rm(sizeof(RelocRec));
    ChainRec *c = new (cm.data()) ChainRec{}; RelocRec *r = new (rm.data()) RelocRec{};
    c->jc.j = 1.0; c->jc.delta[2] = 2.0; c->jc.untestable = 3; c->jc.index[FRAME_MAX - 1] = 4; c->lo.pose[2] = 5.0; c->lo.cov[8] = 6.0; c->lo.chi2 = 7.0; c->lo.status = 8;
    r->pose[2] = 1.0; r->second_pose[2] = 2.0; r->cost = 3.0; r->n_seeds = 4; r->seed[3] = 5; r->status = 6; r->index[FRAME_MAX - 1] = 7; r->e2[FRAME_MAX - 1] = 8.0;
    CHECK(c->jc.index[FRAME_MAX - 1] == 4 && c->lo.status == 8 && r->e2[FRAME_MAX - 1] == 8.0 && r->index[FRAME_MAX - 1] == 7);
    CHECK((unsigned char *)&c->lo.status + 8 == cm.data() + cm.size() && (unsigned char *)&r->e2[FRAME_MAX] == rm.data() + rm.size());
    if (fails == 0) std::printf("frame layout: ok\n");
    return fails ? 1 : 0;
}
