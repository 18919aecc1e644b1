// kernels_layout.hpp -- the kernels that move frame-major data into and out of the row layout (home unit: decoder_layout.hip) and
// the one place their scheme is written down: block order, LDS tile, pad-frame mask, per-dword maps and the row-store side that
// every rows-in kernel shares (llr_labels_in_kernel of kernels_llr.hpp has a load side of its own and ends in rows_from_tile too).
// Templated on PACK (1 = byte rows, 2 = nibble rows; kernels_common.hpp).
//
// A block moves 128 bytes of every frame of one group through LDS as DWORDS (4 nodes of one frame each):
//   global side : 32 lanes x 4 B = 128 contiguous bytes per frame;
//   LDS         : tile[f][c ^ key(f)], key(f) = (f / frames-per-lane) & 31: the XOR swizzle makes both the frame-major side (32
//                 lanes, one frame, all dword columns c) and the row side (lane L reads its own frames 4*PACK*L + k of one column)
//                 hit 32 different banks;
//   registers   : 4x4 byte transposes with v_perm_b32 turn "4 nodes of 4 frames" into "4 frames of one node", the dword a lane
//                 owns in a row (PACK = 2: two of them merged as low / high nibbles).
#pragma once
#include "kernels_common.hpp"

namespace lutldpc {

// XCD-aware block order.  A block moves 128 nodes x one frame group; its frame-major side is one 128-byte
// segment per frame at a stride of N bytes, so unless N is a multiple of 128 every segment straddles two 128-byte lines and
// shares each with the block of the neighbouring node range.  Blocks are dealt round-robin to the 8 XCDs (one L2 each): with the
// plain (x, y) order the two halves of a line are fetched (written) by two different L2s -- measured 3.72 GB read for 2.12 GB of
// input.  Remapped, the blocks of one XCD cover a CONTIGUOUS range of (group, node block): the neighbour that shares a line runs
// on the same XCD a few blocks later and finds it in that L2.
__device__ __forceinline__ void xcd_block(int &bx, int &by) {
    const int gx = (int)gridDim.x, total = gx * (int)gridDim.y, lin = (int)blockIdx.y * gx + (int)blockIdx.x;
    const int per = total / 8;
    int nl = lin;
    if (lin < per * 8) nl = (lin & 7) * per + (lin >> 3);         // (the last total % 8 blocks keep their place)
    bx = nl % gx; by = nl / gx;
}

__device__ __forceinline__ void transpose4x4(uint32_t (&d)[4]) {
    const uint32_t a = __builtin_amdgcn_perm(d[1], d[0], 0x05010400u), b = __builtin_amdgcn_perm(d[1], d[0], 0x07030602u);
    const uint32_t c = __builtin_amdgcn_perm(d[3], d[2], 0x05010400u), e = __builtin_amdgcn_perm(d[3], d[2], 0x07030602u);
    d[0] = __builtin_amdgcn_perm(c, a, 0x05040100u); d[1] = __builtin_amdgcn_perm(c, a, 0x07060302u);
    d[2] = __builtin_amdgcn_perm(e, b, 0x05040100u); d[3] = __builtin_amdgcn_perm(e, b, 0x07060302u);
}

// the tile [frames of a group][32 dword columns], swizzled: dword column c of frame f of the group (frame-major side) ...
template <int PACK>
__device__ __forceinline__ int tile_at(int f, int c) { return f * 32 + (c ^ ((f / (4 * PACK)) & 31)); }
// ... which for the row side, column q of frame 4*PACK*lane + 4h + k (one of the lane's own), is
template <int PACK>
__device__ __forceinline__ int tile_at_lane(int lane, int h, int k, int q) { return (4 * PACK * lane + 4 * h + k) * 32 + (q ^ (lane & 31)); }

// live[h]: 0xFF per frame of the batch, 0x00 per pad frame, for the four frames of half h of the lane's row dword
template <int PACK>
__device__ __forceinline__ void live_frames(uint32_t (&live)[PACK], int g, int lane, int B) {
#pragma unroll
    for (int h = 0; h < PACK; h++) {
        live[h] = 0u;
#pragma unroll
        for (int k = 0; k < 4; k++) if (g * kRowBytes * PACK + 4 * PACK * lane + 4 * h + k < B) live[h] |= 0xFFu << (8 * k);
    }
}

// four labels, one per byte: min(label, lim)
__device__ __forceinline__ uint32_t clamp4(uint32_t x, uint32_t lim) {
    return min(x & 0xFFu, lim) | (min((x >> 8) & 0xFFu, lim) << 8) | (min((x >> 16) & 0xFFu, lim) << 16) | (min(x >> 24, lim) << 24);
}
// a 256-entry byte table held by the wave, four entries per lane (lane L: entries 4L .. 4L+3): entry x through one cross-lane
// read, no memory.  All 64 lanes must be active.
__device__ __forceinline__ uint32_t wave_lut1(uint32_t lutw, uint32_t x) {
    return ((uint32_t)__shfl((int)lutw, (int)(x >> 2), kWave) >> (8 * (x & 3u))) & 0xFFu;
}
__device__ __forceinline__ uint32_t wave_lut4(uint32_t lutw, uint32_t x) {
    return wave_lut1(lutw, x & 0xFFu) | (wave_lut1(lutw, (x >> 8) & 0xFFu) << 8) | (wave_lut1(lutw, (x >> 16) & 0xFFu) << 16) | (wave_lut1(lutw, x >> 24) << 24);
}

// The second half of a rows-in kernel, after the __syncthreads() that completes the tile: the block's dword columns -> rows
// [G][N][256 B] of group g, nodes n0 upwards, stopping at N.  A tile dword holds 4 nodes of a frame, one per byte (NIB = 0), or 8,
// two per byte, even node in bits 0-3 (NIB = 1; split into even and odd nodes in registers, after which each half is "4 nodes of 4
// frames" like byte input).  x = the same node of four frames, one per byte; dst_a gets map_a(x, h), dst_b (TWO = 1) map_b(x, h),
// h = the half of the row dword (PACK = 2: low / high nibbles) the four frames go to.  Every row store is one 256-byte row per
// wave; all 64 lanes are active in the maps.
template <int PACK, int NIB, int TWO, class MapA, class MapB>
__device__ __forceinline__ void rows_from_tile(const uint32_t *tile, int g, int n0, int N, uint8_t *__restrict__ dst_a, uint8_t *__restrict__ dst_b, MapA map_a, MapB map_b)
{
    constexpr int NPC = NIB ? 8 : 4;                        // nodes per dword column
    const int t = threadIdx.x, lane = t & 63;
    for (int q = t >> 6; q < 32; q += 4) {                  // dword column q: nodes n0 + NPC * q .. + NPC - 1
        const int nq = n0 + NPC * q;
        if (nq >= N) break;
        uint32_t a[NPC], b[NPC];
#pragma unroll
        for (int i = 0; i < NPC; i++) a[i] = b[i] = 0u;
#pragma unroll
        for (int h = 0; h < PACK; h++) {
            uint32_t x[NPC];                                // x[i] = node nq + i of frames 4 * PACK * lane + 4h .. + 3, one per byte
            uint32_t d[4];
#pragma unroll
            for (int k = 0; k < 4; k++) d[k] = tile[tile_at_lane<PACK>(lane, h, k, q)];
            if constexpr (NIB) {
                uint32_t lo[4], hi[4];
#pragma unroll
                for (int k = 0; k < 4; k++) { lo[k] = d[k] & 0x0F0F0F0Fu; hi[k] = (d[k] >> 4) & 0x0F0F0F0Fu; }
                transpose4x4(lo); transpose4x4(hi);
#pragma unroll
                for (int j = 0; j < 4; j++) { x[2 * j] = lo[j]; x[2 * j + 1] = hi[j]; }
            } else {
                transpose4x4(d);
#pragma unroll
                for (int j = 0; j < 4; j++) x[j] = d[j];
            }
#pragma unroll
            for (int i = 0; i < NPC; i++) {
                a[i] |= map_a(x[i], h) << (4 * h);
                if constexpr (TWO) b[i] |= map_b(x[i], h) << (4 * h);
            }
        }
#pragma unroll
        for (int i = 0; i < NPC; i++) {
            if (nq + i >= N) break;
            const size_t off = ((size_t)g * N + nq + i) * kRowBytes + lane * 4;
            *reinterpret_cast<uint32_t *>(dst_a + off) = a[i];
            if constexpr (TWO) *reinterpret_cast<uint32_t *>(dst_b + off) = b[i];
        }
    }
}

// ---- labels in ------------------------------------------------------------------------------------
// Frame-major labels -> rows [G][N][256 B], read once; labels are clamped, pad frames get 0:
//   src      frame f at src + f * stride bytes.  NIB = 0: one label per byte (stride = N); NIB = 1: two per byte (stride =
//            ceil(N/2)), node v in byte v/2, even v in bits 0-3, odd v in bits 4-7, the spare nibble of an odd N ignored
//   dst_a    rows of min(label, lim_a)
//   dst_b    TWO = 1: rows of lut_b[label] (a 256-entry device table that holds clamp and map: lut_b[x] = map[min(x, lim_a)])
// A block moves 128 bytes of every frame of one group -- 128 (NIB = 0) or 256 (NIB = 1) nodes -- through the tile as they come.
// VEC = 1: stride % 4 == 0 and src 4-byte aligned, a dword per load; VEC = 0: byte loads with a bound each (odd sizes and bases).
// Bytes that go to one row set only (the byte entries, the benchmark's path) are clamped on their way into the tile, while the
// loads are in flight: clamped after the transposes the layout kernels of the DVB-S2 workload took 2.67 ms per step, so 2.45.
template <int PACK, int NIB, int VEC, int TWO>
__global__ __launch_bounds__(256) void labels_in_kernel(const uint8_t *__restrict__ src, int stride, uint8_t *__restrict__ dst_a,
                                                        uint8_t *__restrict__ dst_b, const uint8_t *__restrict__ lut_b, int B, int N, int lim_a)
{
    constexpr int F = kRowBytes * PACK;                     // frames per group
    constexpr bool kEarly = !TWO && !NIB;
    __shared__ uint32_t tile[F * 32];
    int bx, by;
    xcd_block(bx, by);
    const int g = by, t = threadIdx.x;
    const uint32_t lim = (uint32_t)lim_a;
    const int c = t & 31, fq = t >> 5;
    const int col = bx * 128 + 4 * c;                       // byte offset of this thread's dword inside a frame
    for (int f0 = fq; f0 < F; f0 += 64) {                   // eight loads in flight per thread
        uint32_t v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int fr = g * F + f0 + 8 * j;
            v[j] = 0u;
            if (fr < B) {
                const uint8_t *p = src + ((size_t)fr * stride + col);
                if constexpr (VEC) {
                    if (col < stride) v[j] = *reinterpret_cast<const uint32_t *>(p);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++) if (col + k < stride) v[j] |= (uint32_t)p[k] << (8 * k);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 8; j++) tile[tile_at<PACK>(f0 + 8 * j, c)] = kEarly ? clamp4(v[j], lim) : v[j];
    }
    __syncthreads();
    const bool clamp = !kEarly && !(NIB && lim_a >= 15);    // a nibble cannot exceed the largest label of a 16-label alphabet
    const uint32_t lutw = TWO ? reinterpret_cast<const uint32_t *>(lut_b)[t & 63] : 0u;
    uint32_t live[PACK];                                    // lut_b[0] need not be 0
    live_frames<PACK>(live, g, t & 63, B);
    rows_from_tile<PACK, NIB, TWO>(tile, g, bx * (NIB ? 256 : 128), N, dst_a, dst_b,
                                   [&](uint32_t x, int) { return clamp ? clamp4(x, lim) : x; },
                                   [&](uint32_t x, int h) { return wave_lut4(lutw, x) & live[h]; });
}

// ---- labels out -----------------------------------------------------------------------------------
// rows [G][N][256 B] -> frame-major [B][N], the mirror image: a wave loads the four rows of a dword column, the transposes make
// "4 nodes of one frame" dwords for the tile, and a frame's 128 bytes leave together.  N is the row count of a group (nvar, or the
// edge count for the message trace).  VEC = 1: N % 4 == 0 and dst 4-byte aligned, a dword per store; VEC = 0: the four bytes of a
// tile dword stored one by one and the four rows of a column loaded one by one, with a bound each.  Frames >= B are never written.
template <int PACK, int VEC>
__global__ __launch_bounds__(256) void transpose_out_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int B, int N)
{
    constexpr int F = kRowBytes * PACK;
    __shared__ uint32_t tile[F * 32];
    int bx, by;
    xcd_block(bx, by);
    const int g = by, n0 = bx * 128, t = threadIdx.x;
    const int lane = t & 63;
    for (int q = t >> 6; q < 32; q += 4) {
        const int nq = n0 + 4 * q;
        uint32_t x[4] = {0, 0, 0, 0};
        if (nq < N) {                                        // (VEC = 1: all four rows or none, four loads in flight)
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (VEC || nq + k < N) x[k] = *reinterpret_cast<const uint32_t *>(src + ((size_t)g * N + nq + k) * kRowBytes + lane * 4);
        }
#pragma unroll
        for (int h = 0; h < PACK; h++) {
            uint32_t d[4];
#pragma unroll
            for (int k = 0; k < 4; k++) d[k] = unpack_half<PACK>(x[k], h);
            transpose4x4(d);                                 // d[k] = 4 nodes of frame 4*PACK*lane + 4h + k
#pragma unroll
            for (int k = 0; k < 4; k++) tile[tile_at_lane<PACK>(lane, h, k, q)] = d[k];
        }
    }
    __syncthreads();
    const int c = t & 31, fq = t >> 5;
    for (int f = fq; f < F; f += 8) {
        const int fr = g * F + f, n = n0 + 4 * c;
        if (fr < B && n < N) {
            const uint32_t w = tile[tile_at<PACK>(f, c)];
            uint8_t *p = dst + (size_t)fr * N + n;
            if constexpr (VEC) *reinterpret_cast<uint32_t *>(p) = w;
            else {
#pragma unroll
                for (int k = 0; k < 4; k++) if (n + k < N) p[k] = (uint8_t)(w >> (8 * k));
            }
        }
    }
}

// ---- bits out -------------------------------------------------------------------------------------
// Rows first .. first + count - 1 of the decided-bit rows (bit 0 of a frame's nibble / byte) -> out[B][W] dwords, W =
// ceil(count / 32): bit j of word w of frame f = decided bit first + 32w + j, bits beyond count are 0.  A block makes
// kBitsCols words of every frame of one group: a wave reads the 32 rows of a word (one 256-byte row per load; a row starts
// wherever `first` puts it), merges the bit 0s of 8 / PACK rows into one dword -- the nibble or byte of a frame then holds that
// frame's bits of those rows -- and deals them to the lane's 4 * PACK words; the words cross LDS so that a frame's kBitsCols
// words leave as one contiguous store.  Every output dword is stored whole by one thread; frames >= B are never written.
constexpr int kBitsCols = 16;
template <int PACK>
__global__ __launch_bounds__(256) void packed_bits_out_kernel(const uint8_t *__restrict__ hard, uint32_t *__restrict__ out, int B, int N, int first, int count, int W)
{
    constexpr int F = kRowBytes * PACK, FPL = 4 * PACK;
    constexpr int BITS = 8 / PACK;                          // bits of a frame in a row dword = rows merged per step
    constexpr uint32_t ONES = PACK == 2 ? 0x11111111u : 0x01010101u;
    constexpr int PITCH = F + 4;                            // words of one column in LDS: slot = position in the lane's dword * 64 + lane
    __shared__ uint32_t tile[kBitsCols * PITCH];
    const int g = blockIdx.y, w0 = blockIdx.x * kBitsCols, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int i = 0; i < kBitsCols / 4; i++) {
        const int wc = wave * (kBitsCols / 4) + i, w = w0 + wc;
        uint32_t word[FPL];
#pragma unroll
        for (int p = 0; p < FPL; p++) word[p] = 0u;
        if (w < W) {
#pragma unroll
            for (int r0 = 0; r0 < 32; r0 += BITS) {
                uint32_t m = 0u;
#pragma unroll
                for (int j = 0; j < BITS; j++) {
                    const int bit = 32 * w + r0 + j;
                    uint32_t x = 0u;
                    if (bit < count) x = *reinterpret_cast<const uint32_t *>(hard + ((size_t)g * N + first + bit) * kRowBytes + lane * 4);
                    m |= (x & ONES) << j;
                }
#pragma unroll
                for (int p = 0; p < FPL; p++) word[p] |= ((m >> (BITS * p)) & ((1u << BITS) - 1u)) << r0;
            }
        }
#pragma unroll
        for (int p = 0; p < FPL; p++) tile[wc * PITCH + p * 64 + lane] = word[p];
    }
    __syncthreads();
    const int wc = t & (kBitsCols - 1), w = w0 + wc;
    if (w >= W) return;
    for (int s = t / kBitsCols; s < F; s += 256 / kBitsCols) {
        const int p = s >> 6, L = s & 63;
        // position p of lane L's dword: PACK = 2 -- byte p/2, low nibbles = frames 8L .. 8L+3, high = 8L+4 .. 8L+7; PACK = 1 -- byte p
        const int f = g * F + FPL * L + (PACK == 2 ? 4 * (p & 1) + (p >> 1) : p);
        if (f < B) out[(size_t)f * W + w] = tile[wc * PITCH + s];
    }
}

}  // namespace lutldpc
