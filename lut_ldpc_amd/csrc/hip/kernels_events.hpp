// kernels_events.hpp -- failed frames captured on the device: for every frame of a decoded batch the weight of its residual error
// pattern and of its syndrome, error profiles per node and per check, and -- for the frames a selection rule picks -- one short
// record plus the sorted lists of wrong nodes and unsatisfied checks.  The decided-bit rows never leave the device.
//
// Inputs (after decode_tiles): the decided bits d_hard in tile layout (bit 0 of a frame's nibble / byte), the iteration codes,
// the sent bits as sent-bit rows (kernels_encode.hpp) or none (all-zero codeword).
//
// Work layout.  The N node rows of a frame group are cut into RUNS of rows_per_wave <= 255 rows, the M checks into runs of
// checks_per_wave <= 255 checks; one wave owns one run of one frame group and keeps the counts of its 4*PACK frames per lane in
// byte-wide SWAR accumulators (one dword per half: four frames, one per byte -- 255 rows cannot overflow a byte).
//   event_weights_kernel    row pass: e = (decided ^ sent) & valid frames; per frame cw_errors and data-bit errors (rows < K),
//                           per node the number of wrong frames (ballots + ONE 64-bit atomic per row and frame group)
//   event_syndrome_kernel   the edge walk of syndrome_bits_kernel (eight row loads per step through v_readlane indices) that
//                           COUNTS the closed parities per frame instead of OR-ing a flag; per check the number of failing frames
//   both end with one 32-bit atomic per lane frame that has something to add (as count_errors_kernel) and store the run's
//   accumulators as they are: run_cnt[run][frame] bytes, one coalesced dword store per lane and half.
//   event_select_kernel     one workgroup walks the padded batch in chunks of 1024 frames: selection rule, ballot prefix sum with
//                           a running base -> slots in ascending frame order for ANY B; the first max_frames get their record
//   event_offsets_kernel    per kept frame the exclusive prefix of its run counts: run_off[run][slot]
//   event_fill_*_kernel     the same runs again, kept frames only: a wave whose group keeps no frame returns at once, one whose run
//                           holds nothing to store (no error of a kept frame in it, or all of them beyond max_pos / max_chk)
//                           returns before its first row load; the others write index v / c at run_off + running count.
// Count, scan, fill: every list entry has ONE writer and a position that follows from counts alone, so the lists come out sorted
// and bit-reproducible with plain stores -- no cursors bumped by atomics (arrival order), no sort.  All counters are integers:
// the atomic sums do not depend on the order of arrival either.
#pragma once
#include "kernels_frontend.hpp"

namespace lutldpc {

constexpr int kEvMaxRun = 255;       // rows / checks per run: a frame's count within a run fits a byte
constexpr int kEvRecord = 8;         // int32 per event record

template <int PACK>
__host__ __device__ constexpr uint32_t frame_bit_mask() { return PACK == 2 ? 0x11111111u : 0x01010101u; }
// bit of frame j of a lane inside a row dword (see kernels_common.hpp: half = j / 4, byte = j & 3)
__host__ __device__ constexpr int frame_bit_pos(int j) { return 8 * (j & 3) + 4 * (j >> 2); }

// four bits -> bit 0 of four bytes (bit k lands on k + 7k; the partial products of 1 + 2^7 + 2^14 + 2^21 never meet)
__device__ __forceinline__ uint32_t spread4(uint32_t b) { return ((b & 0xFu) * 0x00204081u) & 0x01010101u; }
// the 4*PACK bits of a lane (bit j = frame j: sent_bits_of_lane) at the frames' bit positions of a row dword
template <int PACK>
__device__ __forceinline__ uint32_t spread_frames(uint32_t b) {
    if constexpr (PACK == 1) return spread4(b);
    else return spread4(b) | (spread4(b >> 4) << 4);
}
// frames of this lane that exist (index < B), as a row-dword mask
template <int PACK>
__device__ __forceinline__ uint32_t valid_frames(int g, int lane, int B) {
    constexpr int F = 4 * PACK;
    int n = B - (g * kWave + lane) * F;
    n = n < 0 ? 0 : n > F ? F : n;
    return spread_frames<PACK>((1u << n) - 1u);
}
// set frame bits of e summed over the wave (wave-uniform result)
template <int PACK>
__device__ __forceinline__ int wave_frame_count(uint32_t e) {
    int n = 0;
#pragma unroll
    for (int j = 0; j < 4 * PACK; j++) n += __popcll(__ballot((e >> frame_bit_pos(j)) & 1u));
    return n;
}
// one atomic per lane frame with a non-zero count; acc[h] = four byte counters (frames 4h .. 4h+3 of the lane)
template <int PACK>
__device__ __forceinline__ void add_lane_frames(int32_t *__restrict__ frame_w, int column, int g, int lane, const uint32_t (&acc)[PACK]) {
#pragma unroll
    for (int j = 0; j < 4 * PACK; j++) {
        const int c = (int)((acc[j / 4] >> (8 * (j & 3))) & 0xFFu);
        if (c) atomicAdd(&frame_w[((size_t)(g * kWave + lane) * (4 * PACK) + j) * 4 + column], c);
    }
}
// run_cnt[run][frame]: the lane's accumulators are its frames' bytes in frame order
template <int PACK>
__device__ __forceinline__ uint32_t *run_cnt_of_lane(uint8_t *run_cnt, int run, int Bpad, int g, int lane) {
    return reinterpret_cast<uint32_t *>(run_cnt + (size_t)run * (size_t)Bpad) + (size_t)(g * kWave + lane) * PACK;
}

// frame_w[f] = {cw_errors, data-bit errors, unsat_checks, -}: zeroed by the caller; this kernel adds columns 0 and 1.
// grid (ceil(ceil(N / rows_per_wave) / 4), G), 256 threads.  sent: sent-bit rows or null.  node_errors / run_cnt: null = not wanted.
template <int PACK>
__global__ __launch_bounds__(256) void event_weights_kernel(const uint8_t *__restrict__ hard, const uint8_t *__restrict__ sent, int B, int Bpad, int N, int K,
                                                            int rows_per_wave, int32_t *__restrict__ frame_w, unsigned long long *__restrict__ node_errors,
                                                            uint8_t *__restrict__ run_cnt)
{
    constexpr int U = 4;                                              // row loads in flight per wave
    const int lane = threadIdx.x & 63, g = blockIdx.y;
    const int w = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const int v0 = w * rows_per_wave;
    int v1 = v0 + rows_per_wave;
    if (v1 > N) v1 = N;
    if (v0 >= v1) return;
    const uint32_t vm = valid_frames<PACK>(g, lane, B);
    const rsrc_t hb = make_rsrc(hard + (size_t)g * (size_t)N * kRowBytes, (uint32_t)N * kRowBytes);
    const uint32_t lane4 = (uint32_t)lane * 4u;
    uint32_t acc[PACK], acc_k[PACK];
#pragma unroll
    for (int h = 0; h < PACK; h++) acc[h] = acc_k[h] = 0;
    for (int vb = v0; vb < v1; vb += U) {
        uint32_t x[U], sb[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const bool in = vb + u < v1;                              // (wave-uniform; a row past the run reads 0 and has no sent bits)
            x[u] = ld_row(hb, (uint32_t)(vb + u) * kRowBytes, lane4 | (in ? 0u : 0x80000000u));
            sb[u] = (sent && in) ? sent_bits_of_lane<PACK>(sent, (size_t)g * N + vb + u, lane) : 0u;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int v = vb + u;
            const uint32_t e = (x[u] ^ spread_frames<PACK>(sb[u])) & vm;
            if (v >= v1 || __ballot(e != 0) == 0ull) continue;
#pragma unroll
            for (int h = 0; h < PACK; h++) {
                const uint32_t t = unpack_half<PACK>(e, h) & 0x01010101u;
                acc[h] += t;
                acc_k[h] += v < K ? t : 0u;
            }
            if (node_errors) {
                const int n = wave_frame_count<PACK>(e);
                if (lane == 0) atomicAdd(&node_errors[v], (unsigned long long)n);
            }
        }
    }
    add_lane_frames<PACK>(frame_w, 0, g, lane, acc);
    add_lane_frames<PACK>(frame_w, 1, g, lane, acc_k);
    if (run_cnt) {
        uint32_t *rc = run_cnt_of_lane<PACK>(run_cnt, w, Bpad, g, lane);
#pragma unroll
        for (int h = 0; h < PACK; h++) rc[h] = acc[h];
    }
}

// Index of the check that closes at check-edge k_last, searched upwards from c (checks without edges are stepped over)
__device__ __forceinline__ int closing_check(const int32_t *__restrict__ cn_ptr, int c, int k_last) {
    while (cn_ptr[c + 1] <= k_last) c++;
    return c;
}

// frame_w column 2 (unsat_checks), check_fails, run_cnt of the check runs.  cn_vnf as in syndrome_bits_kernel: variable node of
// every check-edge, bit 31 on the last edge of its check, padded with eight zero entries.
// grid (ceil(ceil(M / checks_per_wave) / 4), G), 256 threads.
template <int PACK>
__global__ __launch_bounds__(256) void event_syndrome_kernel(const uint8_t *__restrict__ hard, const int32_t *__restrict__ cn_ptr, const uint32_t *__restrict__ cn_vnf,
                                                             int B, int Bpad, int M, int N, int checks_per_wave, int32_t *__restrict__ frame_w,
                                                             unsigned long long *__restrict__ check_fails, uint8_t *__restrict__ run_cnt)
{
    const int lane = threadIdx.x & 63, g = blockIdx.y;
    const int w = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const int c0 = w * checks_per_wave;
    int c1 = c0 + checks_per_wave;
    if (c1 > M) c1 = M;
    if (c0 >= c1) return;
    const uint32_t vm = valid_frames<PACK>(g, lane, B);
    const rsrc_t hb = make_rsrc(hard + (size_t)g * (size_t)N * kRowBytes, (uint32_t)N * kRowBytes);
    const uint32_t lane4 = (uint32_t)lane * 4u;
    const int k0 = cn_ptr[c0], k1 = cn_ptr[c1];
    uint32_t s = 0, acc[PACK];
#pragma unroll
    for (int h = 0; h < PACK; h++) acc[h] = 0;
    int c = c0;
    for (int k = k0; k < k1; k += 8) {
        const uint32_t mine = cn_vnf[k + (lane & 7)];
        uint32_t x[8];
        bool last[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)mine, j);
            last[j] = k + j < k1 && (e >> 31) != 0u;                                             // wave-uniform
            x[j] = ld_row(hb, (e & 0x7FFFFFFFu) * kRowBytes, lane4 | (k + j < k1 ? 0u : 0x80000000u));
        }
#pragma unroll
        for (int j = 0; j < 8; j++) {
            s ^= x[j];
            if (!last[j]) continue;
            const uint32_t closed = s & vm;
            s = 0;
            c = closing_check(cn_ptr, c, k + j);
            if (__ballot(closed != 0) != 0ull) {
#pragma unroll
                for (int h = 0; h < PACK; h++) acc[h] += unpack_half<PACK>(closed, h) & 0x01010101u;
                if (check_fails) {
                    const int n = wave_frame_count<PACK>(closed);
                    if (lane == 0) atomicAdd(&check_fails[c], (unsigned long long)n);
                }
            }
            c++;
        }
    }
    add_lane_frames<PACK>(frame_w, 2, g, lane, acc);
    if (run_cnt) {
        uint32_t *rc = run_cnt_of_lane<PACK>(run_cnt, w, Bpad, g, lane);
#pragma unroll
        for (int h = 0; h < PACK; h++) rc[h] = acc[h];
    }
}

// select: 0 codeword (cw_errors > 0), 1 info (data-bit errors > 0), 2 failed (iteration code < 0), 3 undetected (cw_errors > 0
// and code >= 0).  ONE workgroup of 1024 threads.  slot_of[f] = slot of a kept frame, else -1 (pad frames too);
// events[slot] = {frame, code, cw_errors, data-bit errors, unsat_checks, uncoded errors, positions stored, checks stored};
// counters = {selected, stored}.  stats: the front end's per-frame counters (column 3 = uncoded errors) or null.
__global__ __launch_bounds__(1024) void event_select_kernel(const int32_t *__restrict__ frame_w, const int32_t *__restrict__ iters, const int32_t *__restrict__ stats,
                                                            int B, int Bpad, int select, int max_frames, int max_pos, int max_chk,
                                                            int32_t *__restrict__ events, int32_t *__restrict__ slot_of, int32_t *__restrict__ counters)
{
    __shared__ int wave_sum[16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int base = 0;
    for (int f0 = 0; f0 < Bpad; f0 += 1024) {
        const int f = f0 + (int)threadIdx.x;
        int cw = 0, info = 0, unsat = 0, code = 0;
        bool sel = false;
        if (f < B) {
            cw = frame_w[(size_t)f * 4]; info = frame_w[(size_t)f * 4 + 1]; unsat = frame_w[(size_t)f * 4 + 2]; code = iters[f];
            sel = select == 0 ? cw > 0 : select == 1 ? info > 0 : select == 2 ? code < 0 : (cw > 0 && code >= 0);
        }
        const unsigned long long b = __ballot(sel);
        if (lane == 0) wave_sum[wv] = __popcll(b);
        __syncthreads();
        int before = 0, total = 0;
        for (int i = 0; i < 16; i++) { const int t = wave_sum[i]; before += i < wv ? t : 0; total += t; }
        const int slot = base + before + __popcll(b & ((1ull << lane) - 1ull));
        const bool keep = sel && slot < max_frames;
        if (f < Bpad) slot_of[f] = keep ? slot : -1;
        if (keep) {
            int32_t *r = events + (size_t)slot * kEvRecord;
            r[0] = f; r[1] = code; r[2] = cw; r[3] = info; r[4] = unsat; r[5] = stats ? stats[(size_t)f * 4 + 3] : 0;
            r[6] = cw < max_pos ? cw : max_pos; r[7] = unsat < max_chk ? unsat : max_chk;
        }
        base += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) { counters[0] = base; counters[1] = base < max_frames ? base : max_frames; }
}

// run_off[run][slot] = entries of the kept frame in the runs before `run`.  grid (ceil(cap / 256), 2): y = 0 nodes, 1 checks
// (a null run_cnt: that list is not wanted).  cap = slots allocated (row length of run_off).
__global__ __launch_bounds__(256) void event_offsets_kernel(const int32_t *__restrict__ events, const int32_t *__restrict__ counters, int cap, int Bpad,
                                                            const uint8_t *__restrict__ run_cnt_n, int n_runs_n, int32_t *__restrict__ run_off_n,
                                                            const uint8_t *__restrict__ run_cnt_c, int n_runs_c, int32_t *__restrict__ run_off_c)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= counters[1] || s >= cap) return;
    const uint8_t *cnt = blockIdx.y ? run_cnt_c : run_cnt_n;
    int32_t *off = blockIdx.y ? run_off_c : run_off_n;
    const int n_runs = blockIdx.y ? n_runs_c : n_runs_n;
    if (!cnt) return;
    const int f = events[(size_t)s * kEvRecord];
    int sum = 0;
    for (int r = 0; r < n_runs; r++) {
        off[(size_t)r * cap + s] = sum;
        sum += cnt[(size_t)r * Bpad + f];
    }
}

// What a fill wave knows of its lane's frames: slot[j] (-1: not kept), the next list index cur[j], and `want` = row-dword mask
// of the frames that still have an entry of THIS run to store.  Returns false when the whole wave has none.
template <int PACK>
__device__ __forceinline__ bool fill_prologue(const int32_t *__restrict__ slot_of, const uint8_t *__restrict__ run_cnt, const int32_t *__restrict__ run_off,
                                              int run, int cap, int Bpad, int limit, int g, int lane, int (&slot)[4 * PACK], int (&cur)[4 * PACK], uint32_t &want)
{
    constexpr int F = 4 * PACK;
    uint32_t kept = 0;
#pragma unroll
    for (int j = 0; j < F; j++) {
        slot[j] = slot_of[(size_t)(g * kWave + lane) * F + j];
        kept |= slot[j] >= 0 ? 1u << j : 0u;
    }
    if (__ballot(kept != 0) == 0ull) return false;                    // no kept frame in this frame group
    const uint8_t *cnt = run_cnt + (size_t)run * (size_t)Bpad + (size_t)(g * kWave + lane) * F;
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < F; j++) {
        cur[j] = 0;
        if ((kept >> j) & 1u) {
            cur[j] = run_off[(size_t)run * cap + slot[j]];
            if (cnt[j] != 0 && cur[j] < limit) w |= 1u << frame_bit_pos(j);
        }
    }
    want = w;
    return __ballot(w != 0) != 0ull;
}
template <int PACK>
__device__ __forceinline__ void fill_store(uint32_t e, int index, int limit, const int (&slot)[4 * PACK], int (&cur)[4 * PACK], int32_t *__restrict__ list)
{
#pragma unroll
    for (int j = 0; j < 4 * PACK; j++)
        if ((e >> frame_bit_pos(j)) & 1u) {
            if (cur[j] < limit) list[(size_t)slot[j] * (size_t)limit + cur[j]] = index;
            cur[j]++;
        }
}

// positions[slot][max_pos] (pre-filled with -1): the wrong nodes of every kept frame, ascending.  Grid as event_weights_kernel.
template <int PACK>
__global__ __launch_bounds__(256) void event_fill_nodes_kernel(const uint8_t *__restrict__ hard, const uint8_t *__restrict__ sent, int Bpad, int N, int rows_per_wave,
                                                               const int32_t *__restrict__ slot_of, const uint8_t *__restrict__ run_cnt,
                                                               const int32_t *__restrict__ run_off, int cap, int max_pos, int32_t *__restrict__ positions)
{
    constexpr int F = 4 * PACK;
    const int lane = threadIdx.x & 63, g = blockIdx.y;
    const int w = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const int v0 = w * rows_per_wave;
    int v1 = v0 + rows_per_wave;
    if (v1 > N) v1 = N;
    if (v0 >= v1) return;
    int slot[F], cur[F];
    uint32_t want;
    if (!fill_prologue<PACK>(slot_of, run_cnt, run_off, w, cap, Bpad, max_pos, g, lane, slot, cur, want)) return;
    const rsrc_t hb = make_rsrc(hard + (size_t)g * (size_t)N * kRowBytes, (uint32_t)N * kRowBytes);
    for (int v = v0; v < v1; v++) {
        const uint32_t x = ld_row(hb, (uint32_t)v * kRowBytes, (uint32_t)lane * 4u);
        const uint32_t sb = sent ? sent_bits_of_lane<PACK>(sent, (size_t)g * N + v, lane) : 0u;
        const uint32_t e = (x ^ spread_frames<PACK>(sb)) & want;      // (want holds no pad frame: a pad frame is never kept)
        if (__ballot(e != 0) == 0ull) continue;
        fill_store<PACK>(e, v, max_pos, slot, cur, positions);
    }
}

// checks[slot][max_chk] (pre-filled with -1): the unsatisfied checks of every kept frame, ascending.  Grid as event_syndrome_kernel.
template <int PACK>
__global__ __launch_bounds__(256) void event_fill_checks_kernel(const uint8_t *__restrict__ hard, const int32_t *__restrict__ cn_ptr, const uint32_t *__restrict__ cn_vnf,
                                                                int Bpad, int M, int N, int checks_per_wave, const int32_t *__restrict__ slot_of,
                                                                const uint8_t *__restrict__ run_cnt, const int32_t *__restrict__ run_off, int cap, int max_chk,
                                                                int32_t *__restrict__ checks)
{
    constexpr int F = 4 * PACK;
    const int lane = threadIdx.x & 63, g = blockIdx.y;
    const int w = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const int c0 = w * checks_per_wave;
    int c1 = c0 + checks_per_wave;
    if (c1 > M) c1 = M;
    if (c0 >= c1) return;
    int slot[F], cur[F];
    uint32_t want;
    if (!fill_prologue<PACK>(slot_of, run_cnt, run_off, w, cap, Bpad, max_chk, g, lane, slot, cur, want)) return;
    const rsrc_t hb = make_rsrc(hard + (size_t)g * (size_t)N * kRowBytes, (uint32_t)N * kRowBytes);
    const uint32_t lane4 = (uint32_t)lane * 4u;
    const int k0 = cn_ptr[c0], k1 = cn_ptr[c1];
    uint32_t s = 0;
    int c = c0;
    for (int k = k0; k < k1; k += 8) {
        const uint32_t mine = cn_vnf[k + (lane & 7)];
        uint32_t x[8];
        bool last[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)mine, j);
            last[j] = k + j < k1 && (e >> 31) != 0u;
            x[j] = ld_row(hb, (e & 0x7FFFFFFFu) * kRowBytes, lane4 | (k + j < k1 ? 0u : 0x80000000u));
        }
#pragma unroll
        for (int j = 0; j < 8; j++) {
            s ^= x[j];
            if (!last[j]) continue;
            const uint32_t closed = s & want;
            s = 0;
            c = closing_check(cn_ptr, c, k + j);
            if (__ballot(closed != 0) != 0ull) fill_store<PACK>(closed, c, max_chk, slot, cur, checks);
            c++;
        }
    }
}

}  // namespace lutldpc
