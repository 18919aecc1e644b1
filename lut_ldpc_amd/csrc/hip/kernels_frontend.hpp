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

struct ChannelCells {
    int32_t n_cells;
    int32_t pad;
    uint64_t thr[kMaxCells];       // thr[j] = floor(2^64 * P(cell <= j | bit 0)), j < n_cells-1
    uint8_t cha[kMaxCells];        // labels of each cell when bit 0 was sent
    uint8_t msg[kMaxCells];
    uint8_t neg[kMaxCells];        // 1: x < 0 (slicer decides bit 1)
    uint8_t cha_m[kMaxCells];      // labels of the mirrored cell (bit 1 was sent: x -> -x)
    uint8_t msg_m[kMaxCells];
};

// what an entry samples with: the caller's one table, or the per-node classes the handle holds (sample_labels_classes_kernel)
struct FrontEnd {
    ChannelCells C;
    bool node_classes = false;
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

// cell index = number of thresholds <= u.  The thresholds ascend (checked on the host), so this is an upper-bound
// binary search: 7 steps over the LDS copy of the table instead of up to 71 64-bit compares per sample.  (Used once per
// bucket in the prologue of the sampler; the samples themselves start from their bucket's first cell, below.)
__device__ __forceinline__ int cell_of(const uint64_t *thr_lds, int n_thr, uint64_t u) {
    int lo = 0, n = n_thr;                    // invariant: thr[0..lo) <= u, answer in [lo, lo + n]
#pragma unroll
    for (int step = 0; step < 7; step++) {    // 2^7 > kMaxCells
        const int half = n >> 1;
        const bool right = n > 0 && u >= thr_lds[lo + half];
        lo = right ? lo + half + 1 : lo;
        n = right ? n - half - 1 : half;
    }
    return lo;
}
// The same cell index, found from the sample's BUCKET: the top kBucketBits bits of u select one of 1024 equal slices of the
// unit interval, first_lds[bucket] = number of thresholds <= the slice's lower end, and the few thresholds inside the slice are
// walked one by one (most slices hold none or one; the dense ones sit in the far tails, hit once in ~500 samples).  The
// walk is a wave loop: it ends when no lane advances.  Same result as cell_of for every u.
constexpr int kBucketBits = 10;
__device__ __forceinline__ int cell_from_bucket(const uint64_t *thr_lds, const uint8_t *first_lds, int n_thr, uint64_t u) {
    int cell = first_lds[(uint32_t)(u >> (64 - kBucketBits))];
    for (;;) {
        const bool adv = cell < n_thr && u >= thr_lds[cell < n_thr ? cell : 0];
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
template <int PACK, bool SENT_ROWS = false>
__global__ __launch_bounds__(256) void sample_labels_kernel(const ChannelCells *__restrict__ Cp, uint32_t seed_lo, uint32_t seed_hi, uint32_t stream, uint64_t frame0,
                                                            int B, int N, const uint8_t *__restrict__ sent, uint8_t *__restrict__ cha_t,
                                                            uint8_t *__restrict__ msg_t, int32_t *__restrict__ stats, int pairs_per_thread)
{
    constexpr int F = 4 * PACK;                                     // frames per lane
    __shared__ uint64_t thr_lds[kMaxCells];
    __shared__ uint32_t attr_lds[kMaxCells];                        // per cell: cha | neg << 7 | msg << 8 | cha_m << 16 | msg_m << 24 (labels < 128)
    __shared__ uint8_t first_lds[1 << kBucketBits];
    const ChannelCells &C = *Cp;                                    // (device memory: the argument segment stays small)
    const int n_thr = C.n_cells - 1;
    if (threadIdx.x < kMaxCells) {
        const int t = threadIdx.x < C.n_cells ? threadIdx.x : 0;
        thr_lds[threadIdx.x] = C.thr[threadIdx.x < n_thr ? threadIdx.x : 0];
        attr_lds[threadIdx.x] = (uint32_t)C.cha[t] | ((uint32_t)C.neg[t] << 7) | ((uint32_t)C.msg[t] << 8) | ((uint32_t)C.cha_m[t] << 16) | ((uint32_t)C.msg_m[t] << 24);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < (1 << kBucketBits); t += 256)
        first_lds[t] = (uint8_t)cell_of(thr_lds, n_thr, (uint64_t)t << (64 - kBucketBits));
    __syncthreads();
    const int lane = threadIdx.x & 63, g = blockIdx.y;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int npairs = (N + 1) / 2;
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
        if constexpr (SENT_ROWS) {
#pragma unroll
            for (int hh = 0; hh < 2; hh++)
                if (2 * p + hh < N) sb[hh] = sent_bits_of_lane<PACK>(sent, (size_t)g * N + 2 * p + hh, lane);
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
                const int cell = cell_from_bucket(thr_lds, first_lds, n_thr, u[hh]);
                const int bit = (int)((sb[hh] >> j) & 1u);          // (no sent rows: sb stays zero)
                const uint32_t at = attr_lds[cell], sel = bit ? at >> 16 : at;
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

// ---- per-node channel classes (lutldpc_decoder_set_node_channels): node v is sampled with table node_class[v] -----------------
// One class as the sampler wants it in LDS, made once by the setter: thresholds padded as sample_labels_kernel pads them, the
// packed labels of every cell, the bucket index first[bucket] = number of thresholds <= the bucket's lower end.
constexpr int kMaxNodeClasses = 16;     // LUTLDPC_MAX_NODE_CLASSES: 16 * (576 + 288 + 1024) B = 30208 B of static LDS
struct NodeClassTable {
    uint64_t thr[kMaxCells];
    uint32_t attr[kMaxCells];           // cha | neg << 7 | msg << 8 | cha_m << 16 | msg_m << 24
    uint8_t first[1 << kBucketBits];
    int32_t n_thr, pad;
};
static_assert(sizeof(NodeClassTable) % 8 == 0, "the tables of the classes follow each other as 64-bit words");

// the host twin of the prologue of sample_labels_kernel: C -> its LDS image (first[] by the same upper-bound search)
inline void fill_node_class_table(const ChannelCells &C, NodeClassTable &T) {
    const int n_thr = C.n_cells - 1;
    for (int j = 0; j < kMaxCells; j++) {
        const int t = j < C.n_cells ? j : 0;
        T.thr[j] = C.thr[j < n_thr ? j : 0];
        T.attr[j] = (uint32_t)C.cha[t] | ((uint32_t)C.neg[t] << 7) | ((uint32_t)C.msg[t] << 8) | ((uint32_t)C.cha_m[t] << 16) | ((uint32_t)C.msg_m[t] << 24);
    }
    int cell = 0;
    for (int b = 0; b < (1 << kBucketBits); b++) {
        const uint64_t lo = (uint64_t)b << (64 - kBucketBits);
        while (cell < n_thr && C.thr[cell] <= lo) cell++;          // ascending thresholds: the count never falls from one bucket to the next
        T.first[b] = (uint8_t)cell;
    }
    T.n_thr = n_thr; T.pad = 0;
}

// sample_labels_kernel with the table chosen per node: same grid, same uniforms, same rows and stats.  A wave's lanes are frames
// of ONE node, so the class byte is read once per node as a wave-uniform value and becomes three LDS base offsets; the search of
// a sample is cell_from_bucket on the class's slice.  The prologue copies the LDS images of the classes that occur among the
// workgroup's nodes from device memory (coalesced dwords): no bucket index is built here.  Every class id was checked by the
// setter (< n_classes <= kMaxNodeClasses); nodes beyond N are never looked up.
template <int PACK, bool SENT_ROWS = false>
__global__ __launch_bounds__(256) void sample_labels_classes_kernel(const NodeClassTable *__restrict__ tables, const uint8_t *__restrict__ node_class, uint32_t seed_lo,
                                                                    uint32_t seed_hi, uint32_t stream, uint64_t frame0, int B, int N, const uint8_t *__restrict__ sent,
                                                                    uint8_t *__restrict__ cha_t, uint8_t *__restrict__ msg_t, int32_t *__restrict__ stats, int pairs_per_thread)
{
    constexpr int F = 4 * PACK;                                     // frames per lane
    constexpr int kFirstDwords = (1 << kBucketBits) / 4;
    __shared__ uint64_t thr_lds[kMaxNodeClasses * kMaxCells];
    __shared__ uint32_t attr_lds[kMaxNodeClasses * kMaxCells];
    __shared__ uint32_t first_lds[kMaxNodeClasses * kFirstDwords];
    __shared__ int32_t nthr_lds[kMaxNodeClasses];
    __shared__ uint32_t used_lds;
    const int npairs = (N + 1) / 2;
    if (threadIdx.x == 0) used_lds = 0;
    __syncthreads();
    {   // the classes of the workgroup's nodes: 4 waves x pairs_per_thread pairs, two nodes each
        const int v0 = blockIdx.x * 4 * pairs_per_thread * 2, v1 = min(N, v0 + 4 * pairs_per_thread * 2);
        uint32_t mine = 0;
        for (int v = v0 + (int)threadIdx.x; v < v1; v += 256) mine |= 1u << node_class[v];
        if (mine) atomicOr(&used_lds, mine);
    }
    __syncthreads();
    const uint32_t used = used_lds;
    for (int c = 0; c < kMaxNodeClasses; c++) {
        if (!((used >> c) & 1u)) continue;                          // (workgroup-uniform)
        const NodeClassTable &T = tables[c];
        if (threadIdx.x < kMaxCells) { thr_lds[c * kMaxCells + threadIdx.x] = T.thr[threadIdx.x]; attr_lds[c * kMaxCells + threadIdx.x] = T.attr[threadIdx.x]; }
        first_lds[c * kFirstDwords + threadIdx.x] = reinterpret_cast<const uint32_t *>(T.first)[threadIdx.x];      // 256 threads = 1024 bytes
        if (threadIdx.x == 0) nthr_lds[c] = T.n_thr;
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
        const uint64_t *thr_c[2];
        const uint32_t *attr_c[2];
        const uint8_t *first_c[2];
        int n_thr[2];
#pragma unroll
        for (int hh = 0; hh < 2; hh++) {
            const int v = 2 * p + hh;
            const int cls = v < N ? __builtin_amdgcn_readfirstlane((int)node_class[v]) : 0;      // (the pad node of an odd N is never sampled)
            thr_c[hh] = thr_lds + cls * kMaxCells;
            attr_c[hh] = attr_lds + cls * kMaxCells;
            first_c[hh] = reinterpret_cast<const uint8_t *>(first_lds) + cls * (1 << kBucketBits);
            n_thr[hh] = v < N ? nthr_lds[cls] : 0;
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
                const int cell = cell_from_bucket(thr_c[hh], first_c[hh], n_thr[hh], u[hh]);
                const int bit = (int)((sb[hh] >> j) & 1u);          // (no sent rows: sb stays zero)
                const uint32_t at = attr_c[hh][cell], sel = bit ? at >> 16 : at;
                const uint32_t a = sel & 0x7Fu, m = (sel >> 8) & 0xFFu;
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
