// kernels_encode_sparse.hpp -- the device encoder of codes H = [A | T] whose parity part is (a permutation of) a triangular matrix:
// p = T^-1 (A u), all of it XORs of bit rows.  No dense generator, no limit on K (../host/sparse_generator.hpp builds the arrays).
//
// Bit rows: rows[group][node][RB bytes], RB = 32 * PACK, bit f = the bit of frame f of the group (256 * PACK frames) -- the sent-bit
// row format of kernels_encode.hpp, so an XOR of two nodes is an XOR of two rows.  As dwords a row is DW = RB / 4 = 8 or 16 wide.
//
//   info_rows_random_kernel   information rows from Philox: the bits of encode_random_kernel (same counter, same ballot transposes)
//   info_rows_packed_kernel   information rows from the caller's packed words [B][in_stride] (the input of encode_bits_kernel)
//   sparse_phase_a_kernel     s_i = XOR of the information rows of parity bit i, written to row K + i.  Fully parallel.
//   sparse_phase_b_kernel     p = T^-1 s in place, over the parity-on-parity terms only: a blocked solve.  Blocks of 64 parity bits in
//                             solve order; per block t_k = s_k ^ (finished rows of earlier blocks, from global), t staged in LDS,
//                             p_k = XOR of the t rows that row k of the block's inverse selects (one 64-bit mask, inverted on the
//                             host).  Frames are independent: a workgroup owns a 128-frame slice (4 dwords of every row) through
//                             ALL blocks and needs workgroup barriers only.
//   rows_window_out_kernel    bit rows first .. first+count-1 -> [B][ceil(count/32)] words (the out_words format of encode_packed)
//
// The index lists are wave-uniform wherever one wave works on one row (phase A); in phase B a lane owns (row k of the block, dword).
#pragma once
#include "kernels_encode.hpp"

namespace lutldpc {

constexpr int kSparseBlockRows = 64;          // = lut_ldpc::kSparseBlock (decoder_encode.hip asserts it)
constexpr int kSparseSliceDwords = 4;         // a workgroup of phase B owns 128 frames: 4 dwords of every row
constexpr int kRowsWordChunk = 8;             // consecutive 32-bit words per wave step of the row <-> word kernels

// grid (Bpad / 64, ny), 256 threads.  Wave w of workgroup (x, y) takes the Philox blocks c = 4y + w, 4y + w + 4ny, ...
// Frames >= B get zeros.  rows: at least (Bpad / group_frames) * N * RB bytes.
__global__ __launch_bounds__(256) void info_rows_random_kernel(int K, uint32_t seed_lo, uint32_t seed_hi, uint32_t stream, uint64_t frame0, int B, int N,
                                                               int group_frames, uint8_t *__restrict__ rows)
{
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int W128 = (K + 127) >> 7;
    const int fb = blockIdx.x * 64, fl = fb + lane;
    const uint64_t f = frame0 + (uint64_t)fl;
    const int RB = 32 * (group_frames / 256);
    const int g = fb / group_frames, byte0 = (fb % group_frames) >> 3;
    for (int c = (int)blockIdx.y * 4 + wv; c < W128; c += (int)gridDim.y * 4) {
        const InfoBlock x = info_block(f, c, stream, seed_lo, seed_hi);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint64_t mine = ballot_rows(fl < B ? x.w[j] : 0u, lane);
            const int v = 128 * c + 32 * j + lane;
            if (lane < 32 && v < K) *reinterpret_cast<uint64_t *>(rows + ((size_t)g * N + v) * RB + byte0) = mine;
        }
    }
}

// grid (Bpad / 64, ny), 256 threads.  Wave w of workgroup (x, y) takes the words (4y + w) * 8 .. + 7, then 4 * ny * 8 further on:
// a lane reads consecutive words of its own frame.  Bits >= K are masked, frames >= B get zeros.
__global__ __launch_bounds__(256) void info_rows_packed_kernel(int K, const uint32_t *__restrict__ info, size_t in_stride, int B, int N, int group_frames,
                                                               uint8_t *__restrict__ rows)
{
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int W32 = (K + 31) >> 5;
    const int fb = blockIdx.x * 64, fl = fb + lane;
    const int RB = 32 * (group_frames / 256);
    const int g = fb / group_frames, byte0 = (fb % group_frames) >> 3;
    const uint32_t last_mask = (K & 31) ? (1u << (K & 31)) - 1u : 0xFFFFFFFFu;
    const uint32_t *src = info + (size_t)(fl < B ? fl : 0) * in_stride;
    for (int w0 = ((int)blockIdx.y * 4 + wv) * kRowsWordChunk; w0 < W32; w0 += (int)gridDim.y * 4 * kRowsWordChunk)
        for (int w = w0; w < min(w0 + kRowsWordChunk, W32); w++) {
            uint32_t x = fl < B ? src[w] : 0u;
            if (w == W32 - 1) x &= last_mask;
            const uint64_t mine = ballot_rows(x, lane);
            const int v = 32 * w + lane;
            if (lane < 32 && v < K) *reinterpret_cast<uint64_t *>(rows + ((size_t)g * N + v) * RB + byte0) = mine;
        }
}

// grid (ceil(R / 4), ceil(G / (64 / DW))), 256 threads: one wave = one parity bit i (its term list is wave-uniform: scalar loads)
// over 64 / DW frame groups, lane = (group, dword of the row).  Rows without information terms are written as zeros.
__global__ __launch_bounds__(256) void sparse_phase_a_kernel(const int32_t *__restrict__ a_ptr, const int32_t *__restrict__ a_cols, int K, int R, int N, int G, int DW,
                                                             uint32_t *rows)
{
    const int lane = threadIdx.x & 63;
    const int i = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    if (i >= R) return;
    const int g = (int)blockIdx.y * (64 / DW) + lane / DW, dw = lane % DW;
    if (g >= G) return;
    const uint32_t *base = rows + (size_t)g * N * DW + dw;
    const int beg = a_ptr[i], end = a_ptr[i + 1];
    uint32_t acc = 0;
    for (int e = beg; e < end; e++) acc ^= base[(size_t)a_cols[e] * DW];
    rows[((size_t)g * N + K + i) * DW + dw] = acc;
}

// grid (G * DW / 4), 256 threads: workgroup = (group, 128-frame slice); thread = (k = row of the block, dw = dword of the slice).
// order / e_ptr / inv: Rp = whole blocks of solve positions (pad positions: order -1).  rows is read and written: no __restrict__.
__global__ __launch_bounds__(256) void sparse_phase_b_kernel(const int32_t *__restrict__ order, const int32_t *__restrict__ e_ptr, const int32_t *__restrict__ e_cols,
                                                             const uint64_t *__restrict__ inv, int K, int Rp, int N, int DW, uint32_t *rows)
{
    __shared__ uint32_t t_lds[kSparseBlockRows * kSparseSliceDwords];
    const int slices = DW / kSparseSliceDwords;
    const int g = (int)blockIdx.x / slices, sl = (int)blockIdx.x % slices;
    const int k = threadIdx.x >> 2, dw = threadIdx.x & 3;
    uint32_t *base = rows + ((size_t)g * N + K) * DW + sl * kSparseSliceDwords + dw;      // parity bit i: base[i * DW]
    for (int p0 = 0; p0 < Rp; p0 += kSparseBlockRows) {
        const int p = p0 + k, i = order[p];
        uint32_t t = 0;
        if (i >= 0) {
            t = base[(size_t)i * DW];
            for (int e = e_ptr[p]; e < e_ptr[p + 1]; e++) t ^= base[(size_t)e_cols[e] * DW];
        }
        t_lds[k * kSparseSliceDwords + dw] = t;
        __syncthreads();
        const uint64_t m = inv[p];
        const uint32_t lo = (uint32_t)m, hi = (uint32_t)(m >> 32);
        uint32_t acc = 0;
#pragma unroll
        for (int j = 0; j < 32; j++) {
            acc ^= (0u - ((lo >> j) & 1u)) & t_lds[j * kSparseSliceDwords + dw];
            acc ^= (0u - ((hi >> j) & 1u)) & t_lds[(j + 32) * kSparseSliceDwords + dw];
        }
        if (i >= 0) base[(size_t)i * DW] = acc;
        __syncthreads();          // the rows of this block are read by the next ones; t_lds is free again
    }
}

// grid (ceil(B / 64), ny), 256 threads.  Wave w of workgroup (x, y) takes the output words (4y + w) * 8 .. + 7, then 4 * ny * 8 further
// on.  Lane r < 32 reads the 64 frames of row first + 32w + r; lane l assembles the word of frame l.  Frames >= B are not stored.
__global__ __launch_bounds__(256) void rows_window_out_kernel(const uint8_t *__restrict__ rows, int B, int N, int group_frames, int first, int count,
                                                              uint32_t *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int Wout = (count + 31) >> 5;
    const int fb = blockIdx.x * 64, fl = fb + lane;
    const int RB = 32 * (group_frames / 256);
    const int g = fb / group_frames, byte0 = (fb % group_frames) >> 3;
    for (int w0 = ((int)blockIdx.y * 4 + wv) * kRowsWordChunk; w0 < Wout; w0 += (int)gridDim.y * 4 * kRowsWordChunk)
        for (int w = w0; w < min(w0 + kRowsWordChunk, Wout); w++) {
            const int r = 32 * w + lane;                                   // bit of the window
            uint64_t mine = 0;
            if (lane < 32 && r < count) mine = *reinterpret_cast<const uint64_t *>(rows + ((size_t)g * N + first + r) * RB + byte0);
            const uint32_t lo = (uint32_t)mine, hi = (uint32_t)(mine >> 32);
            uint32_t word = 0;
#pragma unroll
            for (int j = 0; j < 32; j++) {
                const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)lo, j), b = (uint32_t)__builtin_amdgcn_readlane((int)hi, j);
                word |= (((lane < 32 ? a : b) >> (lane & 31)) & 1u) << j;
            }
            if (fl < B) out[(size_t)fl * Wout + w] = word;
        }
}

}  // namespace lutldpc
