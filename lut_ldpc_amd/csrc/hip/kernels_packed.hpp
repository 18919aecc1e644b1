// kernels_packed.hpp -- the layout kernels of lutldpc_decoder_decode_batch_packed (decoder_packed.hip): packed frame-major labels
// into both row sets in one pass, and a window of the decided-bit rows into one bit per frame and node.
// Templated on PACK (1 = byte rows, 2 = nibble rows; kernels_common.hpp) like the transposes of kernels_generic.hpp, whose LDS
// scheme (dword tile, XOR swizzle, 4x4 byte transposes in registers) the label kernel shares.
#pragma once
#include "kernels_common.hpp"
#include "kernels_layout.hpp"

namespace lutldpc {

// ---- labels in ------------------------------------------------------------------------------------
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

// Packed frame-major labels -> rows [G][N][256 B], read once:
//   src      frame f at src + f * stride bytes.  NIB = 0: one label per byte (stride = N); NIB = 1: two per byte (stride =
//            ceil(N/2)), node v in byte v/2, even v in bits 0-3, odd v in bits 4-7, the spare nibble of an odd N ignored
//   dst_a    rows of min(label, lim_a)
//   dst_b    rows of lut_b[label] (a 256-entry device table that holds clamp and map: lut_b[x] = map[min(x, lim_a)]), or null
// Pad frames get 0 in both.  A block moves 128 bytes of every frame of one group -- 128 (NIB = 0) or 256 (NIB = 1) nodes --
// through LDS as dwords, as they come: nibble input stays two labels per byte there and is split into its even and odd nodes in
// registers, after which each half is "4 nodes of 4 frames" and goes through the same 4x4 byte transpose as byte input.
// VEC = 1: stride % 4 == 0 and src 4-byte aligned, a dword per load (32 lanes x 4 B = 128 contiguous bytes per frame); VEC = 0:
// byte loads with a bound each (odd sizes).  Every row store is one 256-byte row per wave.
template <int PACK, int NIB, int VEC>
__global__ __launch_bounds__(256) void packed_labels_in_kernel(const uint8_t *__restrict__ src, size_t stride, uint8_t *__restrict__ dst_a,
                                                               uint8_t *__restrict__ dst_b, const uint8_t *__restrict__ lut_b, int B, int N, int lim_a)
{
    constexpr int F = kRowBytes * PACK, FPL = 4 * PACK;     // frames per group / per lane
    constexpr int NPC = NIB ? 8 : 4;                        // nodes per dword column
    __shared__ uint32_t tile[F * 32];
    int bx, by;
    xcd_block(bx, by);
    const int g = by, n0 = bx * 32 * NPC, t = threadIdx.x;
    const int c = t & 31, fq = t >> 5;
    const size_t col = (size_t)bx * 128 + 4 * (size_t)c;    // byte offset of this thread's dword inside a frame
    for (int f0 = fq; f0 < F; f0 += 64) {                   // eight loads in flight per thread
        uint32_t v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int fr = g * F + f0 + 8 * j;
            v[j] = 0u;
            if (fr < B) {
                const uint8_t *p = src + (size_t)fr * stride + col;
                if constexpr (VEC) {
                    if (col < stride) v[j] = *reinterpret_cast<const uint32_t *>(p);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++) if (col + k < stride) v[j] |= (uint32_t)p[k] << (8 * k);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int f = f0 + 8 * j;
            tile[f * 32 + (c ^ ((f / FPL) & 31))] = v[j];
        }
    }
    __syncthreads();
    const int lane = t & 63;
    const uint32_t lim = (uint32_t)lim_a;
    const bool clamp = !(NIB && lim_a >= 15);               // a nibble cannot exceed the largest label of a 16-label alphabet
    const uint32_t lutw = dst_b ? reinterpret_cast<const uint32_t *>(lut_b)[lane] : 0u;
    uint32_t live[PACK];                                    // 0xFF per frame of the batch, 0x00 per pad frame: lut_b[0] need not be 0
#pragma unroll
    for (int h = 0; h < PACK; h++) {
        live[h] = 0u;
#pragma unroll
        for (int k = 0; k < 4; k++) if (g * F + FPL * lane + 4 * h + k < B) live[h] |= 0xFFu << (8 * k);
    }
    for (int q = t >> 6; q < 32; q += 4) {                  // dword column q: nodes n0 + NPC * q .. + NPC - 1
        const int nq = n0 + NPC * q;
        if (nq >= N) break;
        uint32_t a[NPC], b[NPC];
#pragma unroll
        for (int i = 0; i < NPC; i++) a[i] = b[i] = 0u;
#pragma unroll
        for (int h = 0; h < PACK; h++) {
            uint32_t x[NPC];                                // x[i] = node nq + i of frames FPL * lane + 4h .. + 3, one per byte
            uint32_t d[4];
#pragma unroll
            for (int k = 0; k < 4; k++) d[k] = tile[(FPL * lane + 4 * h + k) * 32 + (q ^ (lane & 31))];
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
                a[i] |= (clamp ? clamp4(x[i], lim) : x[i]) << (4 * h);
                if (dst_b) b[i] |= (wave_lut4(lutw, x[i]) & live[h]) << (4 * h);
            }
        }
#pragma unroll
        for (int i = 0; i < NPC; i++) {
            if (nq + i >= N) break;
            const size_t off = ((size_t)g * N + nq + i) * kRowBytes + lane * 4;
            *reinterpret_cast<uint32_t *>(dst_a + off) = a[i];
            if (dst_b) *reinterpret_cast<uint32_t *>(dst_b + off) = b[i];
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
