// kernels_encode.hpp -- random codewords on the device (zero_codeword = false): the information bits of
// random_info_bits (host/ber_sim_driver.cpp) and the parity of LDPC_Generator_Systematic::encode, for a batch of frames.
//
// Information bits: Philox4x32-10, key = seed, counter = (frame lo, frame hi, k / 128, stream | 0x80000000); output word j
// of block c holds bits 128c + 32j .. 128c + 32j + 31 (bit b = info bit 128c + 32j + b), exactly as on the host.
//
// Parity: parity_i = popcount(A_i & u) mod 2, A = the generator's dense parity rows (R rows over K information bits).  One
// lane = one frame: its info bits sit in LDS (u[c][lane], 16 bytes per Philox block), the A words are wave-uniform (scalar
// loads), so a wave accumulates 32 rows x 32 bits of 64 frames per v_bitop3_b32 (acc ^= a & u) and ends a row with one
// v_bcnt_u32_b32 and a ballot.
//
// Output ("sent-bit rows"): per frame group g (256*PACK frames) and node v one bitmap over the group's frames,
// 32*PACK bytes, bit f = sent bit of frame f of the group.  Lane L of a label row (frames F*L .. F*L+F-1, F = 4*PACK) finds its
// F bits at bit F*L: one byte (PACK = 2) or one nibble (PACK = 1).  Pad frames (>= B) carry zeros.
#pragma once
#include "kernels_frontend.hpp"

namespace lutldpc {

constexpr int kEncFrames = 64;                 // frames per workgroup (one per lane)
constexpr int kEncTileRows = 32;               // parity rows per wave tile (the generator is padded to whole tiles)
constexpr int kEncMaxInfoBits = 64 * 128;      // 64 Philox blocks per frame: 64 KiB of LDS per workgroup

// grid (Bpad / 64, ny), 256 threads, dynamic LDS = ceil(K/128) * 64 * 16 bytes.
// A: Rp = ceil(R/32)*32 rows of W32p = 4*ceil(K/128) dwords, zero beyond R rows / K bits.
// Wave w of workgroup (x, y) takes the parity tiles t = 4y + w, 4y + w + 4ny, ... and the information words likewise.
__global__ __launch_bounds__(256) void encode_random_kernel(const uint32_t *__restrict__ A, int K, int R, int W32p, uint32_t seed_lo, uint32_t seed_hi,
                                                            uint32_t stream, uint64_t frame0, int B, int N, int group_frames, uint8_t *__restrict__ sent)
{
    extern __shared__ uint4 u_lds[];                                   // [c][lane]
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (wave-uniform: the A addresses below go to scalar loads)
    const int W128 = (K + 127) >> 7, W32 = (K + 31) >> 5, T = (R + kEncTileRows - 1) / kEncTileRows;
    const int fb = blockIdx.x * kEncFrames;                            // first frame of the workgroup (batch index)
    const int fl = fb + lane;
    const uint64_t f = frame0 + (uint64_t)fl;
    for (int c = wv; c < W128; c += 4) {
        uint32_t x[4] = {(uint32_t)f, (uint32_t)(f >> 32), (uint32_t)c, stream | 0x80000000u};
        Philox::gen(x, seed_lo, seed_hi);
        u_lds[c * kEncFrames + lane] = fl < B ? make_uint4(x[0], x[1], x[2], x[3]) : make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    const int RB = sent_row_bytes<1>() * (group_frames / 256);        // 32 * PACK
    const int g = fb / group_frames, byte0 = (fb % group_frames) >> 3;  // this wave's 64 frames = 8 bytes of every row
    const int step = (int)gridDim.y * 4, first = (int)blockIdx.y * 4 + wv;
    // information rows: bit b of word w = node 32w + b
    for (int w = first; w < W32; w += step) {
        const uint32_t x = reinterpret_cast<const uint32_t *>(&u_lds[(w >> 2) * kEncFrames + lane])[w & 3];
        uint64_t mine = 0;
#pragma unroll
        for (int b = 0; b < 32; b++) {
            const uint64_t bal = __ballot((x >> b) & 1u);
            mine = lane == b ? bal : mine;
        }
        const int v = 32 * w + lane;
        if (lane < 32 && v < K) *reinterpret_cast<uint64_t *>(sent + ((size_t)g * N + v) * RB + byte0) = mine;
    }
    // parity rows
    for (int t = first; t < T; t += step) {
        const uint32_t *At = A + (size_t)t * kEncTileRows * W32p;
        uint32_t acc[kEncTileRows];
#pragma unroll
        for (int r = 0; r < kEncTileRows; r++) acc[r] = 0;
        for (int c = 0; c < W128; c++) {
            const uint4 u = u_lds[c * kEncFrames + lane];
#pragma unroll
            for (int r = 0; r < kEncTileRows; r++) {
                const uint4 a = *reinterpret_cast<const uint4 *>(At + (size_t)r * W32p + 4 * c);
                // acc ^ (a & u): truth table from acc = 0xF0, a = 0xCC, u = 0xAA
                acc[r] = __builtin_amdgcn_bitop3_b32(acc[r], a.x, u.x, 0x78);
                acc[r] = __builtin_amdgcn_bitop3_b32(acc[r], a.y, u.y, 0x78);
                acc[r] = __builtin_amdgcn_bitop3_b32(acc[r], a.z, u.z, 0x78);
                acc[r] = __builtin_amdgcn_bitop3_b32(acc[r], a.w, u.w, 0x78);
            }
        }
        uint64_t mine = 0;
#pragma unroll
        for (int r = 0; r < kEncTileRows; r++) {
            const uint64_t bal = __ballot(__builtin_popcount(acc[r]) & 1);
            mine = lane == r ? bal : mine;
        }
        const int i = t * kEncTileRows + lane;
        if (lane < kEncTileRows && i < R) *reinterpret_cast<uint64_t *>(sent + ((size_t)g * N + K + i) * RB + byte0) = mine;
    }
}

// sent-bit rows -> frame-major [B][N] bytes (only for callers that want the codewords on the host)
template <int PACK>
__global__ __launch_bounds__(256) void sent_rows_to_bytes_kernel(const uint8_t *__restrict__ rows, int B, int N, uint8_t *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)B * N) return;
    const int f = (int)(i / (size_t)N), v = (int)(i % (size_t)N);
    const int g = f / (256 * PACK), fo = f % (256 * PACK);
    out[i] = (uint8_t)((rows[((size_t)g * N + v) * sent_row_bytes<PACK>() + (fo >> 3)] >> (fo & 7)) & 1u);
}

}  // namespace lutldpc
