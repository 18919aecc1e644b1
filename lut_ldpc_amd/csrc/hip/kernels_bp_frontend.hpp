// kernels_bp_frontend.hpp -- the device front end of the [BP] comparison decoder (include/lut_ldpc_bp.h): the channel as a cell
// sampler that writes the decoder's input rows, and the error counters on its output rows.
//
// Same recipe as the LUT front end (kernels_frontend.hpp): one 64-bit Philox uniform per code bit against integer cumulative
// cell probabilities, integer arithmetic only, the same uniforms.  What differs is the size of the table: a cell per QLLR value,
// some 10^5 of them (150 k at 0 dB, 480 k at 10 dB for rate 1/2 and d1 = 12), 12 bytes each -- 8 for the threshold, 4 for
// qllr << 1 | slicer_neg.  That is 2 to 6 MB: it does not fit the LDS, at low SNR it sits in the 4 MB L2 of an XCD, at high SNR
// in the 256 MB Infinity Cache.  The cell is therefore found in two levels:
//   1. the top kSliceBits bits of u select one of 2^16 equal slices of the unit interval; first[s] = number of thresholds <= the
//      slice's lower end (first[2^16] = all of them), 256 KB, L2-resident;
//   2. the thresholds of the slice, thr[first[s] .. first[s+1]), are searched by bisection.  The trip count is the bit length of
//      their number, fixed before the loop starts.  Around the mean a slice holds a handful of thresholds (2 to 3 trips); the two
//      far-tail slices hold tens of thousands (16 trips), hit by one sample in 2^15 -- a walk would take as many steps as cells.
// The gather is what the kernel costs: each trip is one dependent 8-byte load that a wave issues to up to 64 different lines.  The
// central slices, where nearly all samples fall, span few lines and stay in L2.
//
// Layout as bp_decoder.hip: int32 rows [v][Bpad], thread t of block y = frame 256 y + t, every row access of a wave 256 contiguous
// bytes.  Sent bits arrive frame-major (bytes, bit 0 counts); a block brings a tile of 256 frames x kChunkNodes nodes through the
// LDS so that global reads run along the nodes and the threads read along the frames.
#pragma once
#include "kernels_frontend.hpp"    // Philox

namespace lutldpc {

constexpr int kBpSliceBits = 16;
constexpr int kBpChunkNodes = 64;                  // nodes per tile: 32 Philox blocks per frame

// cell index = number of thresholds <= u (see above); n_thr = 0 (one cell): first is all zero, nothing is read from thr
__device__ __forceinline__ int bp_cell_of(const uint64_t *__restrict__ thr, const uint32_t *__restrict__ first, uint64_t u) {
    const uint32_t s = (uint32_t)(u >> (64 - kBpSliceBits));
    int lo = (int)first[s], n = (int)first[s + 1] - lo;     // invariant: thr[0..lo) <= u, answer in [lo, lo + n]
    const int trips = 32 - __clz(n);                        // n halves (at least) per trip: 0 after bit-length(n) trips
    for (int t = 0; t < trips; t++) {
        const int half = n >> 1;
        const bool right = n > 0 && u >= thr[lo + half];
        lo = right ? lo + half + 1 : lo;
        n = right ? n - half - 1 : half;
    }
    return lo;
}

// tile of sent bits: frames f0 .. f0+255 (those < B), nodes v0 .. v0+kBpChunkNodes-1 (those < N) -> lds[frame][node], padded rows
constexpr int kBpTileStride = kBpChunkNodes + 4;   // bytes per frame in the LDS: 17 dwords, an odd number of banks
__device__ __forceinline__ void bp_load_sent_tile(const uint8_t *__restrict__ cw, uint8_t *lds, int f0, int v0, int B, int N) {
    for (int i = threadIdx.x; i < 256 * kBpChunkNodes; i += 256) {
        const int fr = i / kBpChunkNodes, vv = i % kBpChunkNodes;
        const int f = f0 + fr, v = v0 + vv;
        lds[fr * kBpTileStride + vv] = (f < B && v < N) ? (uint8_t)(cw[(size_t)f * N + v] & 1u) : (uint8_t)0;
    }
}

__global__ __launch_bounds__(256) void bp_zero_kernel(int32_t *__restrict__ p, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0;
}

// rows[v][f] = +-qllr[cell] of frames frame0 .. frame0+B-1 (pad frames: 0), unc[f] += slicer errors of the block's nodes.
// Grid: x = blocks that stride over the chunks of kBpChunkNodes nodes, y = Bpad / 256.  SENT: cw holds the sent bits (never
// null); otherwise the all-zero codeword was sent and cw is not read.
template <bool SENT>
__global__ __launch_bounds__(256) void bp_sample_qllr_kernel(const uint64_t *__restrict__ thr, const int32_t *__restrict__ attr, const uint32_t *__restrict__ first,
                                                             uint32_t seed_lo, uint32_t seed_hi, uint32_t stream, uint64_t frame0, int B, int N, int Bpad,
                                                             const uint8_t *__restrict__ cw, int32_t *__restrict__ rows, int32_t *__restrict__ unc)
{
    __shared__ uint8_t sent_lds[SENT ? 256 * kBpTileStride : 4];
    const int fl = blockIdx.y * 256 + threadIdx.x;                  // frame within the batch, < Bpad
    const uint64_t f = frame0 + (uint64_t)fl;
    const int n_chunks = (N + kBpChunkNodes - 1) / kBpChunkNodes;
    int errs = 0;
    for (int ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
        const int v0 = ch * kBpChunkNodes;
        if constexpr (SENT) {
            __syncthreads();                                        // the tile of the previous chunk has been read
            bp_load_sent_tile(cw, sent_lds, blockIdx.y * 256, v0, B, N);
            __syncthreads();
        }
        const int v1 = v0 + kBpChunkNodes < N ? v0 + kBpChunkNodes : N;
        for (int v = v0; v < v1; v += 2) {                          // v0 is even: (v, v + 1) is the bit pair v / 2
            int q[2] = {0, 0};
            if (fl < B) {
                uint32_t c[4] = {(uint32_t)f, (uint32_t)(f >> 32), (uint32_t)(v >> 1), stream};
                Philox::gen(c, seed_lo, seed_hi);
                const uint64_t u[2] = {((uint64_t)c[1] << 32) | c[0], ((uint64_t)c[3] << 32) | c[2]};
#pragma unroll
                for (int hh = 0; hh < 2; hh++) {
                    if (v + hh >= N) continue;
                    const int a = attr[bp_cell_of(thr, first, u[hh])];
                    errs += a & 1;
                    int bit = 0;
                    if constexpr (SENT) bit = sent_lds[threadIdx.x * kBpTileStride + (v + hh - v0)];
                    q[hh] = bit ? -(a >> 1) : (a >> 1);
                }
            }
            rows[(size_t)v * Bpad + fl] = q[0];
            if (v + 1 < N) rows[(size_t)(v + 1) * Bpad + fl] = q[1];
        }
    }
    if (fl < B && errs) atomicAdd(&unc[fl], errs);
}

// stats[f] = {iters[f], frame error, data bit errors, unc[f]}: the decided bits (out < 0) of the first K nodes against the sent
// ones.  stats is zero on entry; grid as the sampler's, with at least one block in x (K = 0 still reports iters and unc).
template <bool SENT>
__global__ __launch_bounds__(256) void bp_count_errors_kernel(const int32_t *__restrict__ out, const uint8_t *__restrict__ cw, const int32_t *__restrict__ iters,
                                                              const int32_t *__restrict__ unc, int B, int N, int K, int Bpad, int32_t *__restrict__ stats)
{
    __shared__ uint8_t sent_lds[SENT ? 256 * kBpTileStride : 4];
    const int fl = blockIdx.y * 256 + threadIdx.x;
    const int n_chunks = (K + kBpChunkNodes - 1) / kBpChunkNodes;
    int errs = 0;
    for (int ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
        const int v0 = ch * kBpChunkNodes;
        if constexpr (SENT) {
            __syncthreads();
            bp_load_sent_tile(cw, sent_lds, blockIdx.y * 256, v0, B, N);
            __syncthreads();
        }
        const int v1 = v0 + kBpChunkNodes < K ? v0 + kBpChunkNodes : K;
        if (fl < B)
            for (int v = v0; v < v1; v++) {
                int bit = 0;
                if constexpr (SENT) bit = sent_lds[threadIdx.x * kBpTileStride + (v - v0)];
                errs += (out[(size_t)v * Bpad + fl] < 0 ? 1 : 0) ^ bit;
            }
    }
    if (fl >= B) return;
    if (errs) { atomicAdd(&stats[(size_t)fl * 4 + 2], errs); atomicOr(&stats[(size_t)fl * 4 + 1], 1); }
    if (blockIdx.x == 0) { stats[(size_t)fl * 4 + 0] = iters[fl]; stats[(size_t)fl * 4 + 3] = unc[fl]; }
}

}  // namespace lutldpc
