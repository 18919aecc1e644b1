// sparse_generator.hpp -- the host half of the sparse triangular encoder, header-only and free of HIP and of the host classes, so
// that the host library, the device library and a stand-alone check program (tests/sparse_generator_check.cpp) compile the same text.
//
// A code H = [A | T] whose parity part T peels completely (every column of T has, in turn, exactly one entry among the checks
// not yet removed) is encoded through H itself: parity bit K+i = XOR of the other entries of its defining check.  That is a
// sparse triangular system  p = T^-1 (A u)  in place of a dense generator:
//
//   sparse_peel      H (check -> columns, parity columns last) -> CSR: for parity bit K+i the codeword positions whose XOR gives it
//   sparse_order     CSR -> validation, solve order (topological sort), depth of the parity-on-parity dependencies
//   sparse_encode    forward substitution in solve order (host encoder, reference of the device kernels)
//   sparse_pack      CSR + solve order -> the arrays the device kernels read: information terms per parity bit (phase A), and per
//                    block of kSparseBlock parity bits in solve order the terms in earlier blocks and the inverse of the block's own
//                    (triangular, unit diagonal) dependencies as one bit mask per row (phase B)
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace lut_ldpc {

constexpr int kSparseBlock = 64;       // parity bits per block of the blocked solve: one 64-bit inverse row each

struct SparseRows {                    // parity bit K+i = XOR of codeword bits cols[row_ptr[i] .. row_ptr[i+1])
    int K = 0, R = 0;
    std::vector<int32_t> row_ptr, cols;
};

// Peels the columns [K, N) of H: rows[c] = the columns of check c, in the column order the CSR shall speak.  Returns how many of
// the N - K columns peeled; out is complete only where that is all of them (and the number of checks equals N - K).
inline int sparse_peel(int N, int K, const std::vector<std::vector<int>> &rows, SparseRows &out) {
    const int M = (int)rows.size(), R = N - K;
    std::vector<int> count((size_t)(R > 0 ? R : 0), 0), def((size_t)(R > 0 ? R : 0), -1);
    std::vector<std::vector<int>> col_rows((size_t)(R > 0 ? R : 0));
    for (int c = 0; c < M; c++)
        for (int v : rows[(size_t)c])
            if (v >= K && v < N) { count[(size_t)(v - K)]++; col_rows[(size_t)(v - K)].push_back(c); }
    std::vector<char> gone((size_t)M, 0);
    std::vector<int> stack;
    for (int i = 0; i < R; i++) if (count[(size_t)i] == 1) stack.push_back(i);
    int peeled = 0;
    while (!stack.empty()) {
        const int i = stack.back();
        stack.pop_back();
        if (count[(size_t)i] != 1 || def[(size_t)i] >= 0) continue;
        int r = -1;
        for (int c : col_rows[(size_t)i]) if (!gone[(size_t)c]) { r = c; break; }
        if (r < 0) continue;
        def[(size_t)i] = r; gone[(size_t)r] = 1; peeled++;
        for (int v : rows[(size_t)r])
            if (v >= K && v < N && v - K != i && --count[(size_t)(v - K)] == 1) stack.push_back(v - K);
    }
    out = SparseRows();
    if (peeled != R || M != R) return peeled;
    out.K = K; out.R = R;
    out.row_ptr.assign((size_t)R + 1, 0);
    for (int i = 0; i < R; i++) {
        for (int v : rows[(size_t)def[(size_t)i]]) if (v != K + i) out.cols.push_back(v);
        out.row_ptr[(size_t)i + 1] = (int32_t)out.cols.size();
    }
    return peeled;
}

// Validates the CSR and finds a solve order: order[p] = parity bit solved at position p, every parity term of a bit before it.
// Chains stay together (a freed bit is solved next), which keeps their terms inside the block of the blocked solve.
// depth = bits on the longest path of parity-on-parity dependencies (0: R = 0; 1: no parity term anywhere).
// Returns an empty string, or what is wrong.
inline std::string sparse_order(int K, int R, const int32_t *row_ptr, const int32_t *cols, std::vector<int32_t> &order, int &depth) {
    order.clear(); depth = 0;
    if (!row_ptr || !cols) return "NULL array";
    if (K < 1 || R < 0) return "K must be at least 1 and R at least 0";
    if (row_ptr[0] != 0) return "row_ptr must start at 0";
    for (int i = 0; i < R; i++) if (row_ptr[i + 1] < row_ptr[i]) return "row_ptr must ascend (row " + std::to_string(i) + ")";
    const int N = K + R;
    std::vector<int32_t> need((size_t)R, 0), user_ptr((size_t)R + 1, 0);
    for (int i = 0; i < R; i++)
        for (int e = row_ptr[i]; e < row_ptr[i + 1]; e++) {
            const int v = cols[e];
            if (v < 0 || v >= N) return "row " + std::to_string(i) + " names bit " + std::to_string(v) + " outside [0, K + R)";
            if (v == K + i) return "row " + std::to_string(i) + " names its own bit " + std::to_string(v);
            if (v >= K) { need[(size_t)i]++; user_ptr[(size_t)(v - K) + 1]++; }
        }
    for (int i = 0; i < R; i++) user_ptr[(size_t)i + 1] += user_ptr[(size_t)i];
    std::vector<int32_t> users((size_t)user_ptr[(size_t)R]), fill(user_ptr.begin(), user_ptr.end() - 1);
    for (int i = 0; i < R; i++)
        for (int e = row_ptr[i]; e < row_ptr[i + 1]; e++)
            if (cols[e] >= K) users[(size_t)fill[(size_t)(cols[e] - K)]++] = i;
    std::vector<int32_t> level((size_t)R, 1), stack;
    for (int i = R - 1; i >= 0; i--) if (!need[(size_t)i]) stack.push_back(i);          // (popped in ascending order)
    order.reserve((size_t)R);
    while (!stack.empty()) {
        const int i = stack.back();
        stack.pop_back();
        order.push_back(i);
        if (level[(size_t)i] > depth) depth = level[(size_t)i];
        for (int e = user_ptr[(size_t)i + 1] - 1; e >= user_ptr[(size_t)i]; e--) {
            const int u = users[(size_t)e];
            if (level[(size_t)u] < level[(size_t)i] + 1) level[(size_t)u] = level[(size_t)i] + 1;
            if (--need[(size_t)u] == 0) stack.push_back(u);
        }
    }
    if ((int)order.size() != R) {
        int on = -1;                    // a bit still waiting whose every waiting term waits too: walk until a bit repeats
        for (int i = 0; i < R && on < 0; i++) if (need[(size_t)i] > 0) on = i;
        std::vector<char> seen((size_t)R, 0);
        while (!seen[(size_t)on]) {
            seen[(size_t)on] = 1;
            for (int e = row_ptr[on]; e < row_ptr[on + 1]; e++)
                if (cols[e] >= K && need[(size_t)(cols[e] - K)] > 0) { on = cols[e] - K; break; }
        }
        order.clear(); depth = 0;
        return "dependency cycle through bit " + std::to_string(K + on);
    }
    return std::string();
}

// cw[0 .. K) = the information bits; fills cw[K .. K + R)
inline void sparse_encode(int K, int R, const int32_t *row_ptr, const int32_t *cols, const std::vector<int32_t> &order, unsigned char *cw) {
    for (int p = 0; p < R; p++) {
        const int i = order[(size_t)p];
        unsigned char a = 0;
        for (int e = row_ptr[i]; e < row_ptr[i + 1]; e++) a ^= cw[cols[e]];
        cw[K + i] = a & 1;
    }
}

// What the device kernels read.  Solve positions are padded to whole blocks: Rp = ceil(R / block) * block, pad positions
// have order = -1, no terms and an empty inverse row.
struct SparsePacked {
    int K = 0, R = 0, Rp = 0, depth = 0;
    std::vector<int32_t> a_ptr, a_cols;        // phase A, by parity bit: information positions (< K), R + 1 / terms
    std::vector<int32_t> order;                // [Rp] parity bit of solve position p, or -1
    std::vector<int32_t> e_ptr, e_cols;        // phase B, by solve position: parity bits (< R) solved in EARLIER blocks, Rp + 1 / terms
    std::vector<uint64_t> inv;                 // [Rp] row p % block of the inverse of its block: bit j = t of position block0 + j
    int64_t terms() const { return (int64_t)a_cols.size() + (int64_t)e_cols.size() + own_terms; }
    int64_t own_terms = 0;                     // parity terms inside their own block (folded into inv)
};

inline void sparse_pack(int K, int R, const int32_t *row_ptr, const int32_t *cols, const std::vector<int32_t> &order, int depth, SparsePacked &P) {
    static_assert(kSparseBlock == 64, "one uint64_t per inverse row");
    P = SparsePacked();
    P.K = K; P.R = R; P.depth = depth;
    P.Rp = (R + kSparseBlock - 1) / kSparseBlock * kSparseBlock;
    P.a_ptr.assign((size_t)R + 1, 0);
    for (int i = 0; i < R; i++) {
        for (int e = row_ptr[i]; e < row_ptr[i + 1]; e++) if (cols[e] < K) P.a_cols.push_back(cols[e]);
        P.a_ptr[(size_t)i + 1] = (int32_t)P.a_cols.size();
    }
    std::vector<int32_t> pos((size_t)R, 0);
    for (int p = 0; p < R; p++) pos[(size_t)order[(size_t)p]] = p;
    P.order.assign((size_t)P.Rp, -1);
    P.e_ptr.assign((size_t)P.Rp + 1, 0);
    P.inv.assign((size_t)P.Rp, 0);
    for (int p = 0; p < P.Rp; p++) {
        if (p < R) {
            const int i = order[(size_t)p], block0 = p / kSparseBlock * kSparseBlock;
            P.order[(size_t)p] = i;
            uint64_t m = 1ull << (p - block0);
            for (int e = row_ptr[i]; e < row_ptr[i + 1]; e++) {
                if (cols[e] < K) continue;
                const int q = pos[(size_t)(cols[e] - K)];          // (q < p: the order is topological)
                if (q >= block0) { m ^= P.inv[(size_t)q]; P.own_terms++; }
                else P.e_cols.push_back(cols[e] - K);
            }
            P.inv[(size_t)p] = m;
        }
        P.e_ptr[(size_t)p + 1] = (int32_t)P.e_cols.size();
    }
}

// every index the kernels will follow against the arrays they follow it into; empty string = in bounds
inline std::string sparse_packed_check(const SparsePacked &P) {
    if (P.K < 1 || P.R < 0 || P.Rp < P.R || P.Rp % kSparseBlock) return "sizes";
    if ((int)P.a_ptr.size() != P.R + 1 || (int)P.order.size() != P.Rp || (int)P.e_ptr.size() != P.Rp + 1 || (int)P.inv.size() != P.Rp) return "array lengths";
    if (P.a_ptr.front() != 0 || P.a_ptr.back() != (int32_t)P.a_cols.size() || P.e_ptr.front() != 0 || P.e_ptr.back() != (int32_t)P.e_cols.size()) return "CSR ends";
    for (int i = 0; i < P.R; i++) if (P.a_ptr[(size_t)i + 1] < P.a_ptr[(size_t)i]) return "a_ptr descends";
    for (int p = 0; p < P.Rp; p++) if (P.e_ptr[(size_t)p + 1] < P.e_ptr[(size_t)p]) return "e_ptr descends";
    for (int32_t v : P.a_cols) if (v < 0 || v >= P.K) return "information term outside [0, K)";
    for (int32_t v : P.e_cols) if (v < 0 || v >= P.R) return "parity term outside [0, R)";
    for (int p = 0; p < P.Rp; p++) {
        const int32_t i = P.order[(size_t)p];
        if (p < P.R ? (i < 0 || i >= P.R) : i != -1) return "solve order outside [0, R)";
        if (p >= P.R && (P.inv[(size_t)p] || P.e_ptr[(size_t)p + 1] != P.e_ptr[(size_t)p])) return "pad position with terms";
        const int j = p % kSparseBlock;
        if (j < 63 && (P.inv[(size_t)p] >> (j + 1))) return "inverse row above the diagonal";
    }
    return std::string();
}

}  // namespace lut_ldpc
