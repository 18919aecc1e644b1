// Stand-alone check of leading_count_bounds and llr_cell_table (lut_ldpc_amd/csrc/hip/llr_cells.hpp), built and run by
// tests/test_llr_boundaries_cpu.py.  lutldpc_decoder_decode_llr_batch takes boundary arrays as its callers hold them -- unsorted,
// with NaN -- and quantises as quant_nonlin does, by the count of LEADING boundaries below x; the device quantiser counts all
// boundaries below x and needs them non-decreasing.  For seeded arrays of 1..31 boundaries from a small pool (+-inf, NaN, +-0,
// repeats, descending runs) and for NaN, +-inf, +-0, every boundary and its two float64 neighbours as values:
//   * the reference loop on the array as given equals quant_count on leading_count_bounds of it;
//   * the cell of the value (plain count over the thresholds of llr_cell_table, float64, both initial-message modes, a random valid
//     map) looks up the labels the reference loop gives on the arrays as given;
//   * an array that is non-decreasing already comes back bit for bit;
//   * llr_cell_table still refuses an array that is not (its own documented contract) and a map entry equal to Nq_Msg[0].
#include "llr_cells.hpp"

#include <cstdio>
#include <cstring>
#include <limits>
#include <random>

using namespace lutldpc;

static long fails = 0;
#define EXPECT(c, ...) do { if (!(c)) { if (fails++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// quant_nonlin (src/common.cpp:120-129)
static int reference(double x, const std::vector<double> &b) {
    int k = 0;
    for (size_t i = 0; i < b.size(); i++) { if (x > b[i]) k++; else break; }
    return k;
}

static const double kInf = std::numeric_limits<double>::infinity(), kNaN = std::numeric_limits<double>::quiet_NaN();
static const double kPool[] = {-kInf, kInf, kNaN, -0.0, 0.0, -1e30, -3.5, -1.0, -4.9e-324, 4.9e-324, 0.25, 1.0, 1.0 + 2.220446049250313e-16, 2.75, 1e30,
                               1.7976931348623157e308};
constexpr int kPoolN = (int)(sizeof(kPool) / sizeof(kPool[0]));

static std::vector<double> random_bounds(std::mt19937 &rng) {
    std::vector<double> b((size_t)(1 + rng() % 31));
    for (size_t i = 0; i < b.size(); i++) {
        const unsigned how = rng() % 8;
        if (i > 0 && how == 0) b[i] = b[i - 1];                                      // a repeat
        else if (i > 0 && how == 1) b[i] = std::nextafter(b[i - 1], -kInf);          // a descending run, one step at a time
        else b[i] = kPool[rng() % kPoolN];
    }
    return b;
}

static std::vector<double> values_for(const std::vector<double> &a, const std::vector<double> &b) {
    std::vector<double> x = {kNaN, kInf, -kInf, 0.0, -0.0};
    for (const std::vector<double> *v : {&a, &b})
        for (double t : *v) {
            if (std::isnan(t)) continue;
            x.push_back(t); x.push_back(std::nextafter(t, kInf)); x.push_back(std::nextafter(t, -kInf));
        }
    return x;
}

static lutldpc_llr_io io_of(const std::vector<double> &cha, const std::vector<double> &msg, int mode, const std::vector<int32_t> &map) {
    lutldpc_llr_io io{};
    io.dtype = LUTLDPC_LLR_F64;
    io.qb_Cha = cha.data(); io.n_qb_Cha = (int)cha.size();
    if (mode == 0) { io.qb_Msg = msg.data(); io.n_qb_Msg = (int)msg.size(); }
    else io.cha2msg_map = map.data();
    io.initial_message_mode = mode;
    return io;
}

int main(int argc, char **argv) {
    const int n_arrays = argc > 1 ? std::atoi(argv[1]) : 4000;
    std::mt19937 rng(5757);
    long values = 0, unsorted = 0, with_nan = 0;
    for (int it = 0; it < n_arrays; it++) {
        const std::vector<double> cha = random_bounds(rng), msg = random_bounds(rng);
        const std::vector<double> ncha = leading_count_bounds(cha.data(), (int)cha.size()), nmsg = leading_count_bounds(msg.data(), (int)msg.size());
        EXPECT(ncha.size() == cha.size() && nmsg.size() == msg.size(), "array %d: length changed", it);
        bool sorted = true, nan = false;
        for (size_t i = 0; i < cha.size(); i++) { nan |= std::isnan(cha[i]); if (i > 0 && !(cha[i] >= cha[i - 1])) sorted = false; }
        unsorted += !sorted; with_nan += nan;
        const int Nq_Cha = (int)cha.size() + 1, Nq_Msg0 = (int)msg.size() + 1;
        std::vector<int32_t> map((size_t)Nq_Cha);
        for (auto &m : map) m = (int32_t)(rng() % (unsigned)Nq_Msg0);
        LlrCells C[2];
        for (int mode = 0; mode < 2; mode++) {
            const std::string err = llr_cell_table(io_of(ncha, nmsg, mode, map), Nq_Cha, Nq_Msg0, C[mode]);
            EXPECT(err.empty(), "array %d mode %d: refused after the normalisation: %s", it, mode, err.c_str());
            if (!err.empty()) return 1;
        }
        for (double x : values_for(cha, msg)) {
            const int a = reference(x, cha), m = reference(x, msg);
            EXPECT(quant_count(x, ncha.data(), (int)ncha.size()) == a, "array %d: x = %a: channel count %d, reference %d", it, x, quant_count(x, ncha.data(), (int)ncha.size()), a);
            EXPECT(quant_count(x, nmsg.data(), (int)nmsg.size()) == m, "array %d: x = %a: message count %d, reference %d", it, x, quant_count(x, nmsg.data(), (int)nmsg.size()), m);
            for (int mode = 0; mode < 2; mode++) {
                int cell = 0;
                for (int j = 0; j < C[mode].n_thr; j++) cell += x > C[mode].thr[j];
                const int want_msg = mode == 0 ? m : map[(size_t)a];
                EXPECT(C[mode].lut_cha[cell] == a && C[mode].lut_msg[cell] == want_msg, "array %d mode %d: x = %a in cell %d: labels %d %d, reference %d %d", it, mode, x, cell,
                       C[mode].lut_cha[cell], C[mode].lut_msg[cell], a, want_msg);
            }
            values++;
        }
        // the refusals of llr_cell_table itself stay: boundaries as given where they are not in its form, a map entry = Nq_Msg[0]
        LlrCells R;
        if (!sorted || nan) EXPECT(!llr_cell_table(io_of(cha, nmsg, 1, map), Nq_Cha, Nq_Msg0, R).empty(), "array %d: unsorted boundaries accepted as given", it);
        map[rng() % map.size()] = Nq_Msg0;
        EXPECT(!llr_cell_table(io_of(ncha, nmsg, 1, map), Nq_Cha, Nq_Msg0, R).empty(), "array %d: map entry Nq_Msg[0] accepted", it);
        // non-decreasing already (the pool sorted, -0 before +0 or after: both orders are non-decreasing): bit for bit
        std::vector<double> s;
        for (double t : cha) if (!std::isnan(t)) s.push_back(t);
        if (s.empty()) continue;
        std::stable_sort(s.begin(), s.end());
        const std::vector<double> ns = leading_count_bounds(s.data(), (int)s.size());
        EXPECT(ns.size() == s.size() && std::memcmp(ns.data(), s.data(), s.size() * sizeof(double)) == 0, "array %d: a non-decreasing array was changed", it);
    }
    EXPECT(unsorted > n_arrays / 2 && with_nan > n_arrays / 4, "the arrays do not exercise the normalisation: %ld unsorted, %ld with NaN", unsorted, with_nan);
    std::printf("%d arrays (%ld unsorted, %ld with NaN), %ld values checked\n", n_arrays, unsorted, with_nan, values);
    if (fails) { std::printf("%ld failures\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
