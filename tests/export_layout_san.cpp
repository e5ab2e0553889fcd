// export_layout_san.cpp — stand-alone check of csrc/gs_export_host.hpp, the device-layout -> export-layout conversion of
// gs_export_system (structure-of-arrays planes and packed symmetric blocks, the tail arenas with their capacity strides -> array-of-blocks,
// full, row-major).  Every source array is an exact-size heap block filled with values that name (array, plane, index); slots of a tail
// arena beyond the tail's count hold a poison value.  Every exported entry is checked against the index it must come from, every output
// sits between guard cells that must stay untouched, a null output pointer is skipped.  Its own main(), no HIP and no GPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I opendlv-logic-cfsd18-sensation-slam_amd/csrc
//       tests/export_layout_san.cpp -o export_layout_san && ./export_layout_san
#include "gs_export_host.hpp"
#include "gs_host.hpp"           // TAIL_POSES, TAIL_LMS, TAIL_PP, TAIL_PL

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

using namespace gs;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

static const double POISON = -7.0e15, GUARD = 3.0e15;
enum { A_HPP = 1, A_HLL, A_OFF, A_HPL, A_BP, A_BL, T_HPP, T_HLL, T_OFF, T_HPL, T_BP, T_BL };
static double code(int array, int plane, int64_t idx) { return (double)array * 16777216.0 * 16.0 + (double)plane * 16777216.0 + (double)idx; }

// [planes][stride], the first `count` of every plane coded, the rest poison; exact size (a read beyond it is a sanitizer report)
static std::unique_ptr<double[]> planes(int array, int n_planes, int64_t stride, int64_t count) {
    std::unique_ptr<double[]> a(new double[(size_t)(n_planes * stride)]);
    for (int q = 0; q < n_planes; ++q) for (int64_t k = 0; k < stride; ++k) a[(size_t)(q * stride + k)] = k < count ? code(array, q, k) : POISON;
    return a;
}
struct Out {                                                          // n doubles between two guard cells
    std::vector<double> v; size_t n;
    explicit Out(size_t n_) : v(n_ + 2, GUARD), n(n_) { for (size_t k = 0; k < n; ++k) v[k + 1] = POISON; }
    double *p() { return v.data() + 1; }
    double at(size_t k) const { return v[k + 1]; }
    void guards() const { CHECK(v.front() == GUARD && v.back() == GUARD); }
};

static void run(const char *name, int64_t N, int64_t M, int64_t Epp, int64_t L, int64_t baseEpl, int64_t tN, int64_t tM, int64_t tEpp, int64_t tEpl,
                int64_t cN, int64_t cM, int64_t cPP, int64_t cPL, unsigned skip = 0) {
    CHECK(tN <= cN && tM <= cM && tEpp <= cPP && tEpl <= cPL && baseEpl < L);
    const int64_t Epl = baseEpl + tEpl;
    auto Hpp = planes(A_HPP, 6, N, N), Hll = planes(A_HLL, 3, M, M), Off = planes(A_OFF, 9, Epp, Epp), Hpl = planes(A_HPL, 6, L, L);
    auto bp = planes(A_BP, 3, N, N), bl = planes(A_BL, 2, M, M);
    auto tHpp = planes(T_HPP, 6, cN, tN), tHll = planes(T_HLL, 3, cM, tM), tOff = planes(T_OFF, 9, cPP, tEpp), tHpl = planes(T_HPL, 6, cPL, tEpl);
    auto tbp = planes(T_BP, 3, cN, tN), tbl = planes(T_BL, 2, cM, tM);
    // insertion index -> layout index: the base edges scattered over the layout (every 5th outside it), the tail's behind it in order
    std::vector<int32_t> of_ins((size_t)Epl);
    for (int64_t k = 0; k < baseEpl; ++k) of_ins[(size_t)k] = k % 5 == 3 ? -1 : (int32_t)((k * 7 + 2) % L);
    for (int64_t t = 0; t < tEpl; ++t) of_ins[(size_t)(baseEpl + t)] = (int32_t)(L + t);
    Out oHpp((size_t)(N + tN) * 9), oHll((size_t)(M + tM) * 4), oOff((size_t)(Epp + tEpp) * 9), oHpl((size_t)Epl * 6), obp((size_t)(N + tN) * 3), obl((size_t)(M + tM) * 2);
    const ExportCounts c{N, M, Epp, L, Epl, tN, tM, tEpp, tEpl, cN, cM, cPP, cPL};
    const ExportSrc s{Hpp.get(), Hll.get(), Off.get(), Hpl.get(), bp.get(), bl.get(), tHpp.get(), tHll.get(), tOff.get(), tHpl.get(), tbp.get(), tbl.get(), of_ins.data()};
    auto want = [&](int bit, double *p) { return (skip >> bit) & 1u ? nullptr : p; };
    const ExportDst o{want(0, oHpp.p()), want(1, oHll.p()), want(2, oOff.p()), want(3, oHpl.p()), want(4, obp.p()), want(5, obl.p())};
    export_layout(c, s, o);
    static const int sym3[9] = {0, 1, 2, 1, 3, 4, 2, 4, 5}, sym2[4] = {0, 1, 1, 2};
    // vertex and odometry arrays: entry (block v, component q) <- plane pl(q) of the base array at v, or of the tail array at v - base
    auto vertex = [&](const Out &out, int bit, int64_t base, int64_t tail, int width, const int *plane_of, int a_base, int a_tail) {
        out.guards();
        for (int64_t v = 0; v < base + tail; ++v) for (int q = 0; q < width; ++q) { const int pl = plane_of ? plane_of[q] : q;
            const double w = (skip >> bit) & 1u ? POISON : v < base ? code(a_base, pl, v) : code(a_tail, pl, v - base);
            CHECK(out.at((size_t)(v * width + q)) == w); } };
    vertex(oHpp, 0, N, tN, 9, sym3, A_HPP, T_HPP); vertex(oHll, 1, M, tM, 4, sym2, A_HLL, T_HLL); vertex(oOff, 2, Epp, tEpp, 9, nullptr, A_OFF, T_OFF);
    vertex(obp, 4, N, tN, 3, nullptr, A_BP, T_BP); vertex(obl, 5, M, tM, 2, nullptr, A_BL, T_BL);
    oHpl.guards();
    for (int64_t k = 0; k < Epl; ++k) for (int q = 0; q < 6; ++q) { const int64_t e = of_ins[(size_t)k];
        const double w = (skip >> 3) & 1u ? POISON : e < 0 ? 0.0 : e < L ? code(A_HPL, q, e) : code(T_HPL, q, e - L);
        CHECK(oHpl.at((size_t)(k * 6 + q)) == w); }
    std::printf("  %-34s N %lld+%lld M %lld+%lld Epp %lld+%lld Epl %lld+%lld: ok\n", name, (long long)N, (long long)tN, (long long)M, (long long)tM,
                (long long)Epp, (long long)tEpp, (long long)baseEpl, (long long)tEpl);
}

int main() {
    const int64_t cN = TAIL_POSES, cM = TAIL_LMS, cPP = TAIL_PP, cPL = TAIL_PL;
    run("no tail", 70, 30, 74, 281, 170, 0, 0, 0, 0, cN, cM, cPP, cPL);
    run("no tail, no capacity", 70, 30, 74, 281, 170, 0, 0, 0, 0, 0, 0, 0, 0);                       // what gs_export_system passes for an ungrown plan
    run("tail of 1", 70, 30, 74, 281, 170, 1, 1, 1, 1, cN, cM, cPP, cPL);
    run("tail of 1, no new cone", 70, 30, 74, 281, 170, 1, 0, 1, 1, cN, cM, cPP, cPL);
    run("tail of 1 pose, no edge of one kind", 5, 3, 4, 11, 10, 1, 0, 1, 0, cN, cM, cPP, cPL);
    run("tail at capacity", 70, 30, 74, 281, 170, cN, cM, cPP, cPL, cN, cM, cPP, cPL);
    run("capacities larger than counts", 133, 61, 140, 1065, 397, 6, 3, 8, 19, 2 * cN + 1, 3 * cM, cPP + 7, cPL + 13);
    run("counts 1", 1, 1, 1, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1);
    run("base without landmarks or edges", 2, 0, 1, 1, 0, 2, 2, 2, 3, cN, cM, cPP, cPL);
    for (unsigned skip = 1; skip < 64; skip <<= 1) run("one output null", 70, 30, 74, 281, 170, 6, 3, 8, 19, cN, cM, cPP, cPL, skip);
    run("every output null", 70, 30, 74, 281, 170, 6, 3, 8, 19, cN, cM, cPP, cPL, 63);
    std::printf("export layout: ok\n");
    return 0;
}
