// sparse_generator_check -- the host half of the sparse triangular encoder (csrc/host/sparse_generator.hpp) as a stand-alone program,
// meant to be built with -fsanitize=address,undefined: peel, topological sort, block inversion and upload packing on random
// systems, every packed array walked exactly as the device kernels walk it (phase A, then the blocked phase B on 64-frame bit rows)
// and held against plain forward substitution; the refusals of malformed systems.
#include "sparse_generator.hpp"

#include <algorithm>
#include <cstdio>
#include <random>

using namespace lut_ldpc;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fails++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// a random [A | T]: T = a row and column permutation of a unit lower-triangular matrix with `extra` further entries per row
static std::vector<std::vector<int>> random_checks(std::mt19937 &rng, int K, int R, int extra, bool chain) {
    std::vector<int> rp((size_t)R), cp((size_t)R);
    for (int i = 0; i < R; i++) rp[(size_t)i] = cp[(size_t)i] = i;
    std::shuffle(rp.begin(), rp.end(), rng);
    std::shuffle(cp.begin(), cp.end(), rng);
    std::vector<std::vector<int>> rows((size_t)R);
    for (int i = 0; i < R; i++) {
        std::vector<int> &r = rows[(size_t)rp[(size_t)i]];
        r.push_back(K + cp[(size_t)i]);
        if (chain && i) r.push_back(K + cp[(size_t)i - 1]);
        for (int e = 0; e < extra && i && !chain; e++) r.push_back(K + cp[rng() % (unsigned)i]);
        for (int e = 0; e < 3; e++) r.push_back((int)(rng() % (unsigned)K));
        std::sort(r.begin(), r.end());
        r.erase(std::unique(r.begin(), r.end()), r.end());
    }
    return rows;
}

// the kernels' walk over the packed arrays on one 64-frame bit column per node
static std::vector<uint64_t> device_walk(const SparsePacked &P, const std::vector<uint64_t> &info) {
    std::vector<uint64_t> row((size_t)(P.K + P.R), 0);
    std::copy(info.begin(), info.end(), row.begin());
    for (int i = 0; i < P.R; i++) {                                        // phase A
        uint64_t s = 0;
        for (int e = P.a_ptr[(size_t)i]; e < P.a_ptr[(size_t)i + 1]; e++) s ^= row[(size_t)P.a_cols[(size_t)e]];
        row[(size_t)(P.K + i)] = s;
    }
    for (int p0 = 0; p0 < P.Rp; p0 += kSparseBlock) {                      // phase B
        uint64_t t[kSparseBlock];
        for (int k = 0; k < kSparseBlock; k++) {
            const int p = p0 + k, i = P.order[(size_t)p];
            t[k] = 0;
            if (i < 0) continue;
            t[k] = row[(size_t)(P.K + i)];
            for (int e = P.e_ptr[(size_t)p]; e < P.e_ptr[(size_t)p + 1]; e++) t[k] ^= row[(size_t)(P.K + P.e_cols[(size_t)e])];
        }
        for (int k = 0; k < kSparseBlock; k++) {
            const int i = P.order[(size_t)(p0 + k)];
            uint64_t acc = 0;
            for (int j = 0; j < kSparseBlock; j++) if (P.inv[(size_t)(p0 + k)] >> j & 1) acc ^= t[j];
            if (i >= 0) row[(size_t)(P.K + i)] = acc;
        }
    }
    return row;
}

static void one_system(std::mt19937 &rng, int K, int R, int extra, bool chain) {
    const int N = K + R;
    const std::vector<std::vector<int>> rows = random_checks(rng, K, R, extra, chain);
    SparseRows S;
    const int peeled = sparse_peel(N, K, rows, S);
    CHECK(peeled == R && S.K == K && S.R == R && (int)S.row_ptr.size() == R + 1, "peel K %d R %d: %d", K, R, peeled);
    if (peeled != R) return;
    if (S.cols.empty()) S.cols.reserve(1);                                 // (no terms: the pointer must still not be null)
    std::vector<int32_t> order;
    int depth = -1;
    const std::string err = sparse_order(K, R, S.row_ptr.data(), S.cols.data(), order, depth);
    CHECK(err.empty() && (int)order.size() == R, "order K %d R %d: %s", K, R, err.c_str());
    if (!err.empty()) return;
    CHECK(chain ? depth == R : (depth >= (R > 0) && depth <= R), "depth %d of R %d", depth, R);
    SparsePacked P;
    sparse_pack(K, R, S.row_ptr.data(), S.cols.data(), order, depth, P);
    const std::string oob = sparse_packed_check(P);
    CHECK(oob.empty(), "packed arrays K %d R %d: %s", K, R, oob.c_str());
    CHECK(P.terms() == (int64_t)S.cols.size(), "terms %lld of %zu", (long long)P.terms(), S.cols.size());
    std::vector<uint64_t> info((size_t)K);
    for (auto &w : info) w = ((uint64_t)rng() << 32) | rng();
    const std::vector<uint64_t> got = device_walk(P, info);
    for (int f = 0; f < 64; f += 21) {
        std::vector<unsigned char> cw((size_t)N, 0);
        for (int v = 0; v < K; v++) cw[(size_t)v] = (unsigned char)(info[(size_t)v] >> f & 1);
        sparse_encode(K, R, S.row_ptr.data(), S.cols.data(), order, cw.data());
        int bad = 0;
        for (int v = 0; v < N; v++) bad += cw[(size_t)v] != (got[(size_t)v] >> f & 1);
        CHECK(bad == 0, "K %d R %d frame %d: %d bits differ", K, R, f, bad);
        for (const auto &r : rows) {                                       // H c = 0
            int s = 0;
            for (int v : r) s ^= cw[(size_t)v];
            if (s) { CHECK(false, "K %d R %d: a check fails", K, R); break; }
        }
    }
}

static void refusals() {
    std::vector<int32_t> order;
    int depth = 0;
    const int K = 5, R = 4;
    const std::vector<int32_t> rp = {0, 2, 3, 5, 6};
    std::vector<int32_t> cl = {0, K + 1, 1, 2, K + 1, K + 0};
    CHECK(sparse_order(K, R, rp.data(), cl.data(), order, depth).empty() && depth == 3, "valid system refused (depth %d)", depth);
    CHECK(!sparse_order(K, R, nullptr, cl.data(), order, depth).empty() && !sparse_order(K, R, rp.data(), nullptr, order, depth).empty(), "NULL accepted");
    CHECK(!sparse_order(0, R, rp.data(), cl.data(), order, depth).empty() && !sparse_order(K, -1, rp.data(), cl.data(), order, depth).empty(), "bad K / R accepted");
    std::vector<int32_t> bad_rp = rp;
    bad_rp[0] = 1;
    CHECK(!sparse_order(K, R, bad_rp.data(), cl.data(), order, depth).empty(), "row_ptr[0] != 0 accepted");
    bad_rp = rp; bad_rp[2] = 1;
    CHECK(!sparse_order(K, R, bad_rp.data(), cl.data(), order, depth).empty(), "descending row_ptr accepted");
    for (int32_t v : {-1, K + R}) {
        std::vector<int32_t> c = cl;
        c[2] = v;
        CHECK(sparse_order(K, R, rp.data(), c.data(), order, depth).find("outside") != std::string::npos, "entry %d accepted", v);
    }
    std::vector<int32_t> own = cl;
    own[2] = K + 1;
    CHECK(sparse_order(K, R, rp.data(), own.data(), order, depth).find("own bit") != std::string::npos, "own bit accepted");
    std::vector<int32_t> cyc = cl;
    cyc[2] = K + 3;                                                        // 1 -> 3 -> 0 -> 1
    const std::string e = sparse_order(K, R, rp.data(), cyc.data(), order, depth);
    CHECK(e.find("cycle through bit") != std::string::npos && order.empty(), "cycle accepted: %s", e.c_str());
    // a parity part that does not peel: two columns with the same two checks
    SparseRows S;
    CHECK(sparse_peel(4, 2, {{0, 2, 3}, {1, 2, 3}}, S) == 0 && S.row_ptr.empty(), "singular parity part peeled");
}

int main() {
    std::mt19937 rng(20260);
    for (int R : {0, 1, 2, 63, 64, 65, 127, 128, 129, 200, 1000})
        for (int K : {1, 31, 64, 300}) {
            one_system(rng, K, R, 0, false);
            one_system(rng, K, R, 2, false);
            one_system(rng, K, R, 4, false);
            one_system(rng, K, R, 0, true);
        }
    refusals();
    std::printf(fails ? "%d failures\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
