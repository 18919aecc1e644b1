// kernels_stats.hpp -- message-label histograms, counted on the device: how often each label sits on the edges of a dump of
// output_verbosity = 2 / 3 (src/LDPC_Code_LUT.cpp:292-298,311-317,331-337), split by the sent bit of the edge's variable node and
// by a caller-supplied edge grouping.  What density evolution predicts as message densities, measured on a finite-length code.
//
// Work layout (message_histogram_kernel): the edges are sorted by group on the host (lutldpc_decoder_set_edge_groups) and every
// group's run is cut into chunks of kHistChunkMin .. kHistChunkEdges edges; a workgroup owns ONE chunk of ONE frame group, so the group id
// is uniform over the workgroup.  Its waves take the chunk's message rows in turn -- one wave, one 256-byte row, read once with
// ld_row -- and the edge id, its variable node and that node's sent-bit row are wave-uniform.
//
// Counting: every lane owns a column of 32-bit counters in LDS, cnt[wave][sent bit][label][lane] -- lane-private, so the adds are
// plain read-modify-writes without bank conflicts and without atomics (2 * Q * 256 bytes per wave: 8 KB at Q = 16).  A frame
// whose dump is not to be counted (last_dump[f] <= dump: it had left through an exit test in the reference's run, or it is a pad
// frame) adds 0.  At the end of the chunk the workgroup sums its columns, thread b taking bin b of all waves and lanes (the lane
// index rotated by b: conflict-free again), and issues ONE 64-bit atomicAdd per bin it touched.  Integer sums do not depend on
// the order of arrival: the result is bit-reproducible.
#pragma once
#include "kernels_frontend.hpp"

namespace lutldpc {

constexpr int kHistChunkEdges = 512;         // most edges per workgroup (512 rows x 512 frames: a bin's block sum stays far below 2^32)
constexpr int kHistChunkMin = 32;            // fewest (short codes: more workgroups rather than longer ones)
constexpr int kHistLdsPerWave = 32768;       // the workgroup shape keeps waves * 2 * Q * 256 bytes within this (one wave: whatever Q needs)
constexpr int kHistMaxLabels = 128;          // the largest alphabet a decoder can have

// waves per workgroup for an alphabet of Q labels
inline int hist_waves(int Q) { return Q * 512 * 4 <= kHistLdsPerWave ? 4 : Q * 512 * 2 <= kHistLdsPerWave ? 2 : 1; }

// chunks[3c] = {first position in `edges`, number of edges, group id}.  grid (n_chunks, G), hist_waves(Q) * 64 threads,
// dynamic LDS = waves * 2 * Q * 256 bytes.  hist: the slab of this dump, [n_groups][2][n_labels] 64-bit totals.
// sent: sent-bit rows (kernels_encode.hpp) or null = all-zero codeword.  last_dump: per frame of the padded batch.
template <int PACK>
__global__ __launch_bounds__(256) void message_histogram_kernel(const uint8_t *__restrict__ msgs, const int32_t *__restrict__ edges, const int32_t *__restrict__ chunks,
                                                                const int32_t *__restrict__ edge_vn, const uint8_t *__restrict__ sent,
                                                                const int32_t *__restrict__ last_dump, unsigned long long *__restrict__ hist,
                                                                int E, int N, int dump, int Q, int n_labels)
{
    constexpr int F = 4 * PACK;                                       // frames per lane
    extern __shared__ uint32_t hist_cnt[];                            // [wave][2 * Q][64]
    const int lane = threadIdx.x & 63, g = blockIdx.y;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), W = (int)blockDim.x >> 6;
    const int first = chunks[3 * blockIdx.x], count = chunks[3 * blockIdx.x + 1], grp = chunks[3 * blockIdx.x + 2];
    uint32_t *mine = hist_cnt + (size_t)wv * 2 * Q * kWave + lane;    // this lane's column
    for (int b = 0; b < 2 * Q; b++) mine[b * kWave] = 0;
    uint32_t act = 0;                                                 // bit j: frame j of this lane is counted at this dump
#pragma unroll
    for (int j = 0; j < F; j++) act |= (last_dump[(g * kWave + lane) * F + j] > dump ? 1u : 0u) << j;
    if (!wave_all_zero(act)) {
        const rsrc_t rm = make_rsrc(msgs + (size_t)g * E * kRowBytes, (uint32_t)E * kRowBytes);
        for (int k = wv; k < count; k += W) {
            const int e = edges[first + k];
            const uint32_t x = ld_row(rm, (uint32_t)e * kRowBytes, (uint32_t)lane * 4);
            uint32_t sb = 0;
            if (sent) sb = sent_bits_of_lane<PACK>(sent, (size_t)g * N + edge_vn[e], lane);
#pragma unroll
            for (int j = 0; j < F; j++) {
                uint32_t label = (unpack_half<PACK>(x, j / 4) >> (8 * (j & 3))) & 0xFFu;
                label = label < (uint32_t)Q ? label : (uint32_t)Q - 1;            // (a label is below its alphabet; this keeps the column index in range whatever the row holds)
                mine[(((sb >> j) & 1u) * Q + label) * kWave] += (act >> j) & 1u;
            }
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < 2 * Q; b += blockDim.x) {
        uint32_t s = 0;
        for (int w = 0; w < W; w++) {
            const uint32_t *col = hist_cnt + ((size_t)w * 2 * Q + b) * kWave;
            for (int l = 0; l < kWave; l++) s += col[(l + b) & (kWave - 1)];
        }
        if (s) atomicAdd(&hist[((size_t)grp * 2 + b / Q) * n_labels + b % Q], (unsigned long long)s);
    }
}

// How many dumps of a frame are counted: last_dump[f] = that number, a dump k is counted when k < last_dump[f].
// mode 0 (all): every dump of every frame of the batch.  mode 1 (active): the dumps the reference would have PRINTED, from the
// frame's lut_decode return value c -- 0: none; |c| = I: all; 0 < c < I: it returned before the dump of its last variable update,
// after per_iter * c dumps (per_iter = level - 1).  Pad frames: -1.
__global__ __launch_bounds__(256) void last_dump_kernel(const int32_t *__restrict__ iters, int B, int Bpad, int I, int per_iter, int mode, int n_dumps,
                                                        int32_t *__restrict__ last_dump)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= Bpad) return;
    int v = -1;
    if (f < B) {
        const int c = mode ? iters[f] : I;
        v = c == 0 ? 0 : (c > 0 && c < I) ? per_iter * c : n_dumps;
    }
    last_dump[f] = v;
}

}  // namespace lutldpc
