// kernels_encode.hpp -- random codewords on the device (zero_codeword = false): the information bits of
// random_info_bits (host/ber_sim_driver.cpp) and the parity of LDPC_Generator_Systematic::encode, for a batch of frames
// (encode_random_kernel); and the same parity for information bits the caller hands in, bit-packed in and out (encode_bits_kernel).
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

// 32 bits of 64 frames (x of lane l = the word of frame l) -> 32 rows of 64 bits: lane b < 32 returns row b
__device__ __forceinline__ uint64_t ballot_rows(uint32_t x, int lane) {
    uint64_t mine = 0;
#pragma unroll
    for (int b = 0; b < 32; b++) {
        const uint64_t bal = __ballot((x >> b) & 1u);
        mine = lane == b ? bal : mine;
    }
    return mine;
}

// Philox block c of frame f: the information bits 128c .. 128c + 127, word j = bits 128c + 32j ..
struct InfoBlock { uint32_t w[4]; };
__device__ __forceinline__ InfoBlock info_block(uint64_t f, int c, uint32_t stream, uint32_t seed_lo, uint32_t seed_hi) {
    InfoBlock x = {{(uint32_t)f, (uint32_t)(f >> 32), (uint32_t)c, stream | 0x80000000u}};
    Philox::gen(x.w, seed_lo, seed_hi);
    return x;
}

// information word x of the frame of `lane` in u_lds ([c][lane] blocks of 16 bytes) read as dwords
__device__ __forceinline__ int u_word_index(int x, int lane) { return ((x >> 2) * kEncFrames + lane) * 4 + (x & 3); }

// acc[r] = the AND of row r of a 32-row tile with the lane's information bits, folded to one dword (its popcount is the parity
// sum): row(r) = the first dword of row r in A, W128 blocks of four.  Wave-uniform rows: the a words come by scalar loads.
template <class RowOf>
__device__ __forceinline__ void tile_product(uint32_t (&acc)[kEncTileRows], const uint4 *u_lds, int W128, int lane, RowOf row) {
#pragma unroll
    for (int r = 0; r < kEncTileRows; r++) acc[r] = 0;
    for (int c = 0; c < W128; c++) {
        const uint4 u = u_lds[c * kEncFrames + lane];
#pragma unroll
        for (int r = 0; r < kEncTileRows; r++) {
            const uint4 a = *reinterpret_cast<const uint4 *>(row(r) + 4 * c);
            // acc ^ (a & u): truth table from acc = 0xF0, a = 0xCC, u = 0xAA
            acc[r] = __builtin_amdgcn_bitop3_b32(acc[r], a.x, u.x, 0x78);
            acc[r] = __builtin_amdgcn_bitop3_b32(acc[r], a.y, u.y, 0x78);
            acc[r] = __builtin_amdgcn_bitop3_b32(acc[r], a.z, u.z, 0x78);
            acc[r] = __builtin_amdgcn_bitop3_b32(acc[r], a.w, u.w, 0x78);
        }
    }
}

// grid (Bpad / 64, ny), 256 threads, dynamic LDS = ceil(K/128) * 64 * 16 bytes.
// A: Rp = ceil(R/32)*32 rows of W32p = 4*ceil(K/128) dwords, zero beyond R rows / K bits.
// Wave w of workgroup (x, y) takes the parity tiles t = 4y + w, 4y + w + 4ny, ... and the information words likewise.
__global__ __launch_bounds__(256) void encode_random_kernel(const uint32_t *__restrict__ A, int K, int R, int W32p, uint32_t seed_lo, uint32_t seed_hi,
                                                            uint32_t stream, uint64_t frame0, int B, int N, int group_frames, uint8_t *__restrict__ sent)
{
    extern __shared__ uint4 u_lds[];                                   // [c][lane]
    const uint32_t *u_words = reinterpret_cast<const uint32_t *>(u_lds);
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (wave-uniform: the A addresses below go to scalar loads)
    const int W128 = (K + 127) >> 7, W32 = (K + 31) >> 5, T = (R + kEncTileRows - 1) / kEncTileRows;
    const int fb = blockIdx.x * kEncFrames;                            // first frame of the workgroup (batch index)
    const int fl = fb + lane;
    const uint64_t f = frame0 + (uint64_t)fl;
    for (int c = wv; c < W128; c += 4) {
        const InfoBlock x = info_block(f, c, stream, seed_lo, seed_hi);
        u_lds[c * kEncFrames + lane] = fl < B ? make_uint4(x.w[0], x.w[1], x.w[2], x.w[3]) : make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    const int RB = sent_row_bytes<1>() * (group_frames / 256);        // 32 * PACK
    const int g = fb / group_frames, byte0 = (fb % group_frames) >> 3;  // this wave's 64 frames = 8 bytes of every row
    const int step = (int)gridDim.y * 4, first = (int)blockIdx.y * 4 + wv;
    // information rows: bit b of word w = node 32w + b
    for (int w = first; w < W32; w += step) {
        const uint64_t mine = ballot_rows(u_words[u_word_index(w, lane)], lane);
        const int v = 32 * w + lane;
        if (lane < 32 && v < K) *reinterpret_cast<uint64_t *>(sent + ((size_t)g * N + v) * RB + byte0) = mine;
    }
    // parity rows
    for (int t = first; t < T; t += step) {
        const uint32_t *At = A + (size_t)t * kEncTileRows * W32p;
        uint32_t acc[kEncTileRows];
        tile_product(acc, u_lds, W128, lane, [&](int r) { return At + (size_t)r * W32p; });
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

// The caller's information bits -> codewords, both bit-packed and frame-major (lutldpc_decoder_encode_packed): the arithmetic of
// encode_random_kernel (one lane = one frame, u[c][lane] in LDS, wave-uniform A words, acc ^= a & u, popcount parity) with loads in
// place of Philox and words in place of sent-bit rows.
//
// info: [B][in_stride] dwords, bit j of word w = information bit 32w + j; words ceil(K/32) .. in_stride-1 are never read, bits at
// positions >= K of the last word are masked.  A wave reads consecutive words of one frame (coalesced dwords) and writes them to
// that frame's column of u_lds: the LDS write is the transposition.  Frames >= B load nothing (zeros in LDS) and store nothing.
//
// out: [B][Wout] dwords, Wout = ceil(out_count/32); bit j of word w = codeword bit out_first + 32w + j, zero beyond out_count.
// The 32-row tiles are aligned to the OUTPUT words: the wave that owns word w (c0 = out_first + 32w) takes the information bits
// c0 .. min(K, c0+32)-1 from LDS (a funnel shift of two words) and computes the parity rows max(0, c0-K) .. min(R, c0+32-K)-1, which land
// at bit max(0, K-c0) upwards: K % 32 != 0 and any out_first are that one shift.  A lane owns its frame, so it assembles the word
// from its own 32 parities and stores it once: no ballot, no atomics, no word written by two waves.  Rows past the tile's last
// one are read from the row Rp-1 at most (the generator's pad rows keep that in bounds) and masked off; words below K need no A.
//
// grid (ceil(B/64), ny), 256 threads, dynamic LDS = ceil(K/128) * 64 * 16 bytes (as encode_random_kernel).  Wave w of workgroup
// (x, y) takes the output words 4y + w, 4y + w + 4ny, ...
__global__ __launch_bounds__(256) void encode_bits_kernel(const uint32_t *__restrict__ A, int K, int R, int W32p, const uint32_t *__restrict__ info,
                                                          size_t in_stride, int B, int out_first, int out_count, uint32_t *__restrict__ out)
{
    extern __shared__ uint4 u_lds[];                                   // [c][lane]
    uint32_t *u_words = reinterpret_cast<uint32_t *>(u_lds);
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (wave-uniform: the A addresses below go to scalar loads)
    const int W128 = (K + 127) >> 7, W32 = (K + 31) >> 5, Rp = (R + kEncTileRows - 1) / kEncTileRows * kEncTileRows;
    const int Wout = (out_count + 31) >> 5;
    const int fb = blockIdx.x * kEncFrames;                            // first frame of the workgroup
    const int fl = fb + lane;
    const uint32_t last_mask = (K & 31) ? (1u << (K & 31)) - 1u : 0xFFFFFFFFu;
    // frame fb + j of the workgroup: wave j % 4 reads its words lane, lane + 64, ...; the spare words of the last block are zero
    for (int j = wv; j < kEncFrames; j += 4) {
        const bool live = fb + j < B;                                  // (wave-uniform)
        const uint32_t *src = info + (size_t)(fb + j) * in_stride;
        for (int x = lane; x < 4 * W128; x += 64) {
            uint32_t v = 0;
            if (live && x < W32) v = src[x] & (x == W32 - 1 ? last_mask : 0xFFFFFFFFu);
            u_words[u_word_index(x, j)] = v;
        }
    }
    __syncthreads();
    const int step = (int)gridDim.y * 4, first = (int)blockIdx.y * 4 + wv;
    for (int w = first; w < Wout; w += step) {
        const int c0 = out_first + 32 * w;                             // codeword bit at bit 0 of this word
        uint32_t word = 0;
        if (c0 < K) {                                                  // information bits c0 .. : words x0, x0 + 1 shifted down by s
            const int x0 = c0 >> 5, s = c0 & 31;
            const uint32_t lo = u_words[u_word_index(x0, lane)];
            const uint32_t hi = (s && x0 + 1 < W32) ? u_words[u_word_index(x0 + 1, lane)] : 0u;
            word = s ? (lo >> s) | (hi << (32 - s)) : lo;
        }
        const int jlo = c0 < K ? K - c0 : 0;                           // bit of the first parity row of this word (>= 32: none)
        const int r0 = c0 < K ? 0 : c0 - K;                            // that row
        const int nrows = min(R - r0, 32 - jlo);                       // rows r0 .. r0 + nrows - 1 (wave-uniform)
        if (jlo < 32 && nrows > 0) {
            uint32_t acc[kEncTileRows];
            uint32_t roff[kEncTileRows];                               // row i of the tile in A; past the tile: a row in bounds, masked below
#pragma unroll
            for (int i = 0; i < kEncTileRows; i++) roff[i] = (uint32_t)min(r0 + i, Rp - 1) * (uint32_t)W32p;
            tile_product(acc, u_lds, W128, lane, [&](int i) { return A + roff[i]; });
            uint32_t par = 0;
#pragma unroll
            for (int i = 0; i < kEncTileRows; i++) par |= (uint32_t)(__builtin_popcount(acc[i]) & 1) << i;
            if (nrows < 32) par &= (1u << nrows) - 1u;
            word |= par << jlo;
        }
        const int left = out_count - 32 * w;                           // bits of the window in this word
        if (left < 32) word &= (1u << left) - 1u;
        if (fl < B) out[(size_t)fl * Wout + w] = word;
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

// frame-major codewords [B][N] (bytes 0 / 1) -> sent-bit rows: the inverse of sent_rows_to_bytes_kernel.  One thread per byte of
// the rows (eight frames of one node); pad frames get zeros.
template <int PACK>
__global__ __launch_bounds__(256) void bytes_to_sent_rows_kernel(const uint8_t *__restrict__ cw, int B, int N, size_t n_bytes, uint8_t *__restrict__ rows)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_bytes) return;
    constexpr int RB = sent_row_bytes<PACK>();
    const size_t row = i / RB;                                        // g * N + v
    const int g = (int)(row / (size_t)N), v = (int)(row % (size_t)N), f0 = g * 256 * PACK + (int)(i % RB) * 8;
    uint32_t b = 0;
#pragma unroll
    for (int k = 0; k < 8; k++)
        if (f0 + k < B) b |= (uint32_t)(cw[(size_t)(f0 + k) * N + v] & 1u) << k;
    rows[i] = (uint8_t)b;
}

}  // namespace lutldpc
