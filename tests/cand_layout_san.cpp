// cand_layout_san.cpp — a stand-alone program (its own main, no HIP) around csrc/gs_cand_host.hpp, built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_cand_cpu.py.  It carves the two tables and the stage out of a heap block of exactly
// CandLayout::bytes, and a batch call's uploads and outputs out of one of exactly CandBatch::bytes for every size such a call can ask for,
// and writes every piece to its last byte, as the kernels and the copies do: a piece that overlaps its neighbour, leaves the block or breaks
// its alignment is found here.  The frame call's staging is filled the same way at its largest.
#include "gs_cand_host.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace gs;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

struct Piece { size_t off, bytes, align; unsigned char tag; };

static void fill(std::vector<unsigned char> &mem, const std::vector<Piece> &ps) {
    for (const Piece &p : ps) { CHECK(p.off % 256 == 0 && p.off % p.align == 0); CHECK(p.off + p.bytes <= mem.size());
        if (p.bytes && p.off + p.bytes <= mem.size()) std::memset(mem.data() + p.off, p.tag, p.bytes); }
    for (const Piece &p : ps)                                                  // nobody wrote into anybody else
        for (size_t b = 0; b < p.bytes && p.off + b < mem.size(); ++b) if (mem[p.off + b] != p.tag) { CHECK(!"a piece was overwritten"); break; }
}

static void tables() {
    CandLayout L; cand_layout(L);
    std::vector<unsigned char> mem(L.bytes, 0);
    std::vector<Piece> ps; unsigned char tag = 1;
    for (int s = 0; s < 2; ++s) { const size_t t = L.table[s];
        ps.push_back({t + L.xy, (size_t)CAND_MAX * 16, 16, tag++}); ps.push_back({t + L.type, (size_t)CAND_MAX * 4, 4, tag++});
        ps.push_back({t + L.cov, (size_t)CAND_MAX * 32, 32, tag++}); ps.push_back({t + L.rec, (size_t)CAND_MAX * CAND_REC_BYTES, 8, tag++});
        ps.push_back({t + L.meta, 16, 4, tag++}); }
    ps.push_back({L.st_obs, (size_t)CAND_FRAME_MAX * 32, 32, tag++}); ps.push_back({L.st_pose_of_obs, (size_t)CAND_FRAME_MAX * 4, 4, tag++});
    ps.push_back({L.st_fs, 8, 4, tag++}); ps.push_back({L.as_idx, (size_t)CAND_FRAME_MAX * 4, 4, tag++});
    ps.push_back({L.as_d2, (size_t)CAND_FRAME_MAX * 8, 8, tag++}); ps.push_back({L.as_na, (size_t)CAND_FRAME_MAX * 4, 4, tag++});
    CHECK(L.table[1] == L.table[0] + L.table_bytes && L.st_obs >= 2 * L.table_bytes);
    fill(mem, ps);
}

static void batch(long long n_steps, long long n, long long n_in) {
    CandBatch B;
    CHECK(cand_batch_layout(n_steps, n, n_in, B));
    std::vector<unsigned char> mem(B.bytes, 0);
    const size_t ns = (size_t)n_steps, no = (size_t)n;
    fill(mem, {{B.obs, no * 32, 32, 1}, {B.fs, (ns + 1) * 4, 4, 2}, {B.pose, ns * 24, 8, 3}, {B.cov, ns * 72, 8, 4}, {B.in_idx, no * 4, 4, 5},
               {B.in_table, (size_t)n_in * CAND_REC_BYTES, 8, 6}, {B.steps, ns * CAND_STEP_BYTES, 4, 7}, {B.out_id, no * 4, 4, 8}, {B.out_slot, no * 4, 4, 9}});
}

int main() {
    tables();
    CandBatch B;
    CHECK(!cand_batch_layout(-1, 0, 0, B) && !cand_batch_layout(0, -1, 0, B) && !cand_batch_layout(0, 0, -1, B) && !cand_batch_layout(0, 0, CAND_MAX + 1, B));
    const long long steps[] = {0, 1, 2, 12, 33}, obs[] = {0, 1, 63, 256, 3000}, ins[] = {0, 1, 1023, 1024};
    for (long long s : steps) for (long long n : obs) for (long long i : ins) batch(s, n, i);
    using Io = CandFrameIo;
    CHECK(Io::IN_OBS % 32 == 0 && Io::IN_COV >= Io::IN_POSE + 24 && Io::IN_FS >= Io::IN_COV + 72 && Io::IN_IDX >= Io::IN_FS + 8);
    CHECK(Io::IN_OBS >= Io::IN_IDX + (size_t)CAND_FRAME_MAX * 4 && Io::in_bytes(CAND_FRAME_MAX) == Io::IN_BYTES && Io::in_bytes(0) == Io::IN_OBS);
    CHECK(Io::OUT_STEP >= Io::IN_BYTES && Io::OUT_ID >= Io::OUT_STEP + CAND_STEP_BYTES && Io::OUT_ID % 4 == 0 && Io::OUT_SLOT == Io::OUT_ID + (size_t)CAND_FRAME_MAX * 4);
    CHECK(Io::BYTES == Io::OUT_SLOT + (size_t)CAND_FRAME_MAX * 4);
    std::vector<unsigned char> io(Io::BYTES);
    std::memset(io.data() + Io::IN_OBS, 1, (size_t)CAND_FRAME_MAX * 32);
    std::memset(io.data() + Io::OUT_SLOT, 2, (size_t)CAND_FRAME_MAX * 4);
    if (fails == 0) std::printf("cand layout: ok\n");
    return fails ? 1 : 0;
}
