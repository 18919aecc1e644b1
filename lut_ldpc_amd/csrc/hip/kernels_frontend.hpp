// kernels_frontend.hpp -- Monte-Carlo front end on the device: the per-frame work of
// LDPC_BER_Sim::sim_snr_point (src/LDPC_BER_Sim.cpp:260-286) other than the decode itself.
//
// The reference draws N Gaussian samples per frame, forms LLR = 4x/N0 and quantises them
// (BPSK + AWGN_Channel + demodulate_soft_bits + quant_nonlin).  All the decoder ever sees of a
// received value x is (channel label, initial message label, slicer sign), i.e. which cell of the
// partition of the real line by the thresholds {qb_Cha*N0/4} u {qb_Msg*N0/4} u {0} it fell
// into.  The sampler therefore draws the CELL directly: one 64-bit uniform per code bit is
// compared against the integer cumulative cell probabilities (computed once per SNR point on the
// host from the Gaussian cdf).  This is an exact sampler of the same joint distribution (up to
// the 2^-64 resolution of the thresholds), needs no transcendental on the device and -- because
// everything after the thresholds is integer arithmetic -- gives bit-identical label streams on
// the GPU and in the CPU oracle.  (The IT++ random stream itself cannot be reproduced: SURVEY F5.)
//
// Random numbers: Philox4x32-10 (Salmon et al., SC'11), key = seed, counter =
// (frame index lo, hi, code-bit pair index, stream id); the four output words give the two
// 64-bit uniforms of code bits 2p and 2p+1.  Frames are therefore addressable: any sharding of
// the frame range over GPUs produces the same frames.
#pragma once
#include "kernels_common.hpp"

namespace lutldpc {

constexpr int kMaxCells = 72;      // 2*(Nq-1)+1 thresholds for Nq <= 32 ... generous

constexpr int kBucketBits = 10;    // the top bits of a uniform select one of 1024 equal slices of the unit interval (cell_from_bucket)
constexpr int kMaxNodeClasses = 16; // LUTLDPC_MAX_NODE_CLASSES: 16 tables of 1896 B = 30336 B of LDS

// One cell table (lutldpc_channel_cells) as the sampler reads it, in device memory and, copied verbatim, in LDS.  Made on the host
// by the one builder (decoder_frontend.hip: fill_table); entries past the table's own are zero.
struct NodeClassTable {
    uint64_t thr[kMaxCells];            // thr[j] = floor(2^64 * P(cell <= j | bit 0)), j < n_thr
    // per cell: cha | neg << 7 | msg << 8 | cha_m << 16 | msg_m << 24 -- the labels when bit 0 was sent (< 128), neg = 1: x < 0 (the
    // slicer decides bit 1), the labels of the mirrored cell (bit 1 was sent: x -> -x)
    uint32_t attr[kMaxCells];
    uint8_t first[1 << kBucketBits];    // first[bucket] = number of thresholds <= the bucket's lower end
    int32_t n_thr, pad;                 // n_cells - 1
};
static_assert(sizeof(NodeClassTable) % 8 == 0, "the tables of the classes follow each other as 64-bit words");

// first[s] = how many of the n ascending thresholds are <= s << (64 - BITS), the lower end of slice s of the 2^BITS equal slices
// of the unit interval: one merge, the count never falls from one slice to the next
template <int BITS, class T>
inline void slice_index(const uint64_t *thr, int n, T *first) {
    int k = 0;
    for (int s = 0; s < (1 << BITS); s++) {
        while (k < n && thr[k] <= (uint64_t)s << (64 - BITS)) k++;
        first[s] = (T)k;
    }
}

// what an entry samples with, as sample_labels_kernel takes it: the caller's one table (one slot, no class bytes) or the per-node
// classes the handle holds (lutldpc_decoder_set_node_channels); all device memory
struct FrontEnd {
    const NodeClassTable *tables = nullptr;
    const uint8_t *node_class = nullptr;
    int n_slots = 0;
};

struct Philox {
    __host__ __device__ static inline void round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    }
    __host__ __device__ static inline void gen(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
        for (int r = 0; r < 10; r++) {
            round(c, k0, k1);
            k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
        }
    }
};

// cell index = number of thresholds <= u (they ascend: checked on the host), found from the sample's BUCKET: the top kBucketBits
// bits of u select one of 1024 equal slices of the unit interval, T.first[bucket] = number of thresholds <= the slice's lower
// end, and the few thresholds inside the slice are walked one by one (most slices hold none or one; the dense ones sit in the
// far tails, hit once in ~500 samples).  The walk is a wave loop: it ends when no lane advances.  T: a table in LDS.
__device__ __forceinline__ int cell_from_bucket(const NodeClassTable &T, int n_thr, uint64_t u) {
    int cell = T.first[(uint32_t)(u >> (64 - kBucketBits))];
    for (;;) {
        const bool adv = cell < n_thr && u >= T.thr[cell < n_thr ? cell : 0];
        if (!__any(adv)) break;
        cell += adv ? 1 : 0;
    }
    return cell;
}

// Sent-bit rows (kernels_encode.hpp, codewords made on the device): per frame group and node a bitmap over the group's
// 256*PACK frames, 32*PACK bytes; lane L of a label row finds the bits of its frames F*L .. F*L+F-1 at bit F*L.
template <int PACK>
__host__ __device__ constexpr int sent_row_bytes() { return 32 * PACK; }
template <int PACK>
__device__ __forceinline__ uint32_t sent_bits_of_lane(const uint8_t *__restrict__ rows, size_t row, int lane) {
    const uint32_t b = rows[row * sent_row_bytes<PACK>() + ((lane * 4 * PACK) >> 3)];
    if constexpr (PACK == 2) return b;
    else return (b >> ((lane & 1) * 4)) & 0xFu;
}

// Writes cha_t / msg0_t rows (row layout) for B frames starting at global frame index frame0 and
// adds the slicer errors of each frame to stats[f][3].  One thread = 4*PACK frames x a run of
// code-bit pairs.  SENT_ROWS: the sent bits are the sent-bit rows `sent` (never null); otherwise the
// all-zero codeword was sent and `sent` is not read.
// Node v is sampled with table node_class[v] of the n_slots `tables` (device memory: the argument segment stays small); a null
// node_class is class 0 on every node, the caller's one table.  The tables live in dynamic LDS, n_slots * sizeof(NodeClassTable)
// bytes, slot = class id; the prologue copies the images of the classes that occur among the workgroup's nodes (coalesced dwords).
// A wave's lanes are frames of ONE node, so the class byte is read once per node as a wave-uniform value and selects the slot.
// Every class id was checked by the setter (< n_classes = n_slots <= kMaxNodeClasses); nodes beyond N are never looked up.
template <int PACK, bool SENT_ROWS = false>
__global__ __launch_bounds__(256) void sample_labels_kernel(const NodeClassTable *__restrict__ tables, const uint8_t *__restrict__ node_class, int n_slots, uint32_t seed_lo,
                                                            uint32_t seed_hi, uint32_t stream, uint64_t frame0, int B, int N, const uint8_t *__restrict__ sent,
                                                            uint8_t *__restrict__ cha_t, uint8_t *__restrict__ msg_t, int32_t *__restrict__ stats, int pairs_per_thread)
{
    constexpr int F = 4 * PACK;                                     // frames per lane
    constexpr int kTableDwords = sizeof(NodeClassTable) / 4;
    extern __shared__ __attribute__((aligned(16))) NodeClassTable table_lds[];
    __shared__ uint32_t used_lds;
    const int npairs = (N + 1) / 2;
    uint32_t used = 1;
    if (node_class) {   // the classes of the workgroup's nodes: 4 waves x pairs_per_thread pairs, two nodes each
        if (threadIdx.x == 0) used_lds = 0;
        __syncthreads();
        const int v0 = blockIdx.x * 4 * pairs_per_thread * 2, v1 = min(N, v0 + 4 * pairs_per_thread * 2);
        uint32_t mine = 0;
        for (int v = v0 + (int)threadIdx.x; v < v1; v += 256) mine |= 1u << node_class[v];
        if (mine) atomicOr(&used_lds, mine);
        __syncthreads();
        used = used_lds;
    }
    for (int c = 0; c < n_slots; c++) {
        if (!((used >> c) & 1u)) continue;                          // (workgroup-uniform)
        const uint32_t *src = reinterpret_cast<const uint32_t *>(tables + c);
        uint32_t *dst = reinterpret_cast<uint32_t *>(table_lds + c);
        for (int i = threadIdx.x; i < kTableDwords; i += 256) dst[i] = src[i];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, g = blockIdx.y;
    const int w = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int p0 = w * pairs_per_thread, p1 = p0 + pairs_per_thread;
    if (p1 > npairs) p1 = npairs;
    int unc[F];
#pragma unroll
    for (int j = 0; j < F; j++) unc[j] = 0;
    for (int p = p0; p < p1; p++) {
        uint32_t ca[2][PACK], ms[2][PACK];
#pragma unroll
        for (int h = 0; h < PACK; h++) { ca[0][h] = ca[1][h] = 0; ms[0][h] = ms[1][h] = 0; }
        uint32_t sb[2] = {0u, 0u};
        const NodeClassTable *T[2];
        int n_thr[2];
#pragma unroll
        for (int hh = 0; hh < 2; hh++) {
            const int v = 2 * p + hh;
            const int cls = node_class && v < N ? __builtin_amdgcn_readfirstlane((int)node_class[v]) : 0;      // (the pad node of an odd N is never sampled)
            T[hh] = table_lds + cls;
            n_thr[hh] = v < N ? T[hh]->n_thr : 0;
            if constexpr (SENT_ROWS) { if (v < N) sb[hh] = sent_bits_of_lane<PACK>(sent, (size_t)g * N + v, lane); }
        }
#pragma unroll
        for (int j = 0; j < F; j++) {
            const int fl = (g * kWave + lane) * F + j;              // frame within the batch
            if (fl >= B) continue;                                  // pad frames keep label 0
            const uint64_t f = frame0 + (uint64_t)fl;
            uint32_t c[4] = {(uint32_t)f, (uint32_t)(f >> 32), (uint32_t)p, stream};
            Philox::gen(c, seed_lo, seed_hi);
            const uint64_t u[2] = {((uint64_t)c[1] << 32) | c[0], ((uint64_t)c[3] << 32) | c[2]};
#pragma unroll
            for (int hh = 0; hh < 2; hh++) {
                const int v = 2 * p + hh;
                if (v >= N) continue;
                const int cell = cell_from_bucket(*T[hh], n_thr[hh], u[hh]);
                const int bit = (int)((sb[hh] >> j) & 1u);          // (no sent rows: sb stays zero)
                const uint32_t at = T[hh]->attr[cell], sel = bit ? at >> 16 : at;
                const uint32_t a = sel & 0x7Fu, m = (sel >> 8) & 0xFFu;
                // slicer decision: neg for bit 0, its mirror for bit 1 -- wrong exactly when the cell lies on the negative side
                unc[j] += (int)((at >> 7) & 1u);
                ca[hh][j / 4] |= a << (8 * (j & 3));
                ms[hh][j / 4] |= m << (8 * (j & 3));
            }
        }
#pragma unroll
        for (int hh = 0; hh < 2; hh++) {
            const int v = 2 * p + hh;
            if (v >= N) continue;
            *reinterpret_cast<uint32_t *>(cha_t + ((size_t)g * N + v) * kRowBytes + lane * 4) = pack_halves<PACK>(ca[hh]);
            *reinterpret_cast<uint32_t *>(msg_t + ((size_t)g * N + v) * kRowBytes + lane * 4) = pack_halves<PACK>(ms[hh]);
        }
    }
#pragma unroll
    for (int j = 0; j < F; j++) {
        const int fl = (g * kWave + lane) * F + j;
        if (fl < B && unc[j]) atomicAdd(&stats[(size_t)fl * 4 + 3], unc[j]);
    }
}

// stats[f] = {iteration code, frame error, data bit errors, uncoded bit errors}: compares the decided
// bits of the first K positions with the sent ones (BERC / BLERC of src/LDPC_BER_Sim.cpp:284-286);
// SENT_ROWS: as in sample_labels_kernel
template <int PACK, bool SENT_ROWS = false>
__global__ __launch_bounds__(256) void count_errors_kernel(const uint8_t *__restrict__ hard, const uint8_t *__restrict__ sent, int B, int N, int K,
                                                           const int32_t *__restrict__ iters, int32_t *__restrict__ stats, int rows_per_wave)
{
    constexpr int F = 4 * PACK;
    const int lane = threadIdx.x & 63, g = blockIdx.y;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    int v0 = w * rows_per_wave, v1 = v0 + rows_per_wave;
    if (v1 > K) v1 = K;
    int err[F];
#pragma unroll
    for (int j = 0; j < F; j++) err[j] = 0;
    for (int v = v0; v < v1; v++) {
        const uint32_t x = *reinterpret_cast<const uint32_t *>(hard + ((size_t)g * N + v) * kRowBytes + lane * 4);
        uint32_t sb = 0;
        if constexpr (SENT_ROWS) sb = sent_bits_of_lane<PACK>(sent, (size_t)g * N + v, lane);
#pragma unroll
        for (int j = 0; j < F; j++) {
            const uint32_t hw = unpack_half<PACK>(x, j / 4);
            err[j] += (int)(((hw >> (8 * (j & 3))) ^ (sb >> j)) & 1u);      // (pad frames and no sent rows: zeros)
        }
    }
#pragma unroll
    for (int j = 0; j < F; j++) {
        const int fl = (g * kWave + lane) * F + j;
        if (fl < B && err[j]) { atomicAdd(&stats[(size_t)fl * 4 + 2], err[j]); atomicOr(&stats[(size_t)fl * 4 + 1], 1); }
        if (fl < B && v0 == 0) stats[(size_t)fl * 4 + 0] = iters[fl];
    }
}

}  // namespace lutldpc
