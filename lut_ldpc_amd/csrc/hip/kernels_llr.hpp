// kernels_llr.hpp -- the layout kernel of the two LLR entries (decoder_llr.hip): frame-major soft values quantised
// straight into both label row sets, read once.  Block order, tile and the whole store side (rows_from_tile) are the shared ones of
// kernels_layout.hpp; only the load side is this kernel's own.  What goes through the tile here is the CELL of a value
// (llr_cells.hpp), one byte, from which two wave-held tables give both labels.
#pragma once
#include "kernels_common.hpp"
#include "kernels_layout.hpp"

namespace lutldpc {

// device copy of the tables of one call (LlrCells): the thresholds in the type the kernel compares in
struct LlrTables {
    uint8_t lut_cha[256], lut_msg[256];
    union { double f64[255]; float f32[255]; } thr;
};

// the type a value is compared in: float16 widens exactly to float (a half denormal is a float normal), int8 is never compared
template <class T> struct LlrCmp { using type = float; };
template <> struct LlrCmp<double> { using type = double; };

// four consecutive elements, loaded as a whole where base and stride allow it (at most 16 bytes per load instruction)
template <class T>
struct alignas(sizeof(T) * 4 > 16 ? 16 : sizeof(T) * 4) LlrQuad { T v[4]; };

// Frame-major values -> rows [G][N][256 B] of lut_cha[cell] and of lut_msg[cell]:
//   src     frame f at src + f * stride elements of T (double, float, _Float16, int8_t); elements >= N of a frame are never read
//   tab     the tables; n_thr thresholds, ascending.  cell = #{j : x > thr[j]} (NaN: 0); int8: the byte itself
// A block moves 128 nodes of every frame of one group.  A thread loads four consecutive nodes of eight frames, counts the
// thresholds below each of the 32 values (the thresholds are wave-uniform: scalar loads, one per threshold for all 32) and
// stores the four cell bytes of a frame as one dword into the tile.  Nodes >= N and frames >= B stage 0.
// VEC = 1: stride % 4 == 0 and src aligned to an LlrQuad, one quad per load (32 lanes x 4 elements contiguous per frame); VEC = 0:
// element loads with a bound each (odd strides and bases).  The last quad of a frame whose N is no multiple of 4 is loaded by
// elements in both.  The two maps handed to rows_from_tile are the wave-held tables, both masked with `live`: pad frames get
// label 0 in both (lut_cha[0] is not 0 for int8).
template <int PACK, class T, int VEC>
__global__ __launch_bounds__(256) void llr_labels_in_kernel(const T *__restrict__ src, size_t stride, uint8_t *__restrict__ dst_cha, uint8_t *__restrict__ dst_msg,
                                                            const LlrTables *__restrict__ tab, int n_thr, int B, int N)
{
    using TC = typename LlrCmp<T>::type;
    constexpr bool kBytes = sizeof(T) == 1;
    constexpr int F = kRowBytes * PACK;                     // frames per group
    __shared__ uint32_t tile[F * 32];
    int bx, by;
    xcd_block(bx, by);
    const int g = by, n0 = bx * 128, t = threadIdx.x;
    const int c = t & 31, fq = t >> 5;
    const int n = n0 + 4 * c;                               // first of this thread's four nodes
    for (int f0 = fq; f0 < F; f0 += 64) {                   // eight loads in flight per thread
        LlrQuad<T> v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int fr = g * F + f0 + 8 * j;
#pragma unroll
            for (int k = 0; k < 4; k++) v[j].v[k] = T(0);
            if (fr < B && n < N) {
                const T *p = src + (size_t)fr * stride + n;
                if (VEC && n + 3 < N) v[j] = *reinterpret_cast<const LlrQuad<T> *>(p);
                else {
#pragma unroll
                    for (int k = 0; k < 4; k++) if (n + k < N) v[j].v[k] = p[k];
                }
            }
        }
        uint32_t cell[8][4];
        if constexpr (kBytes) {
#pragma unroll
            for (int j = 0; j < 8; j++)
#pragma unroll
                for (int k = 0; k < 4; k++) cell[j][k] = (uint32_t)(uint8_t)v[j].v[k];
        } else {
            TC x[8][4];
#pragma unroll
            for (int j = 0; j < 8; j++)
#pragma unroll
                for (int k = 0; k < 4; k++) { x[j][k] = (TC)v[j].v[k]; cell[j][k] = 0u; }
            const TC *thr = reinterpret_cast<const TC *>(&tab->thr);
#pragma unroll 1
            for (int i = 0; i < n_thr; i++) {
                const TC u = thr[i];
#pragma unroll
                for (int j = 0; j < 8; j++)
#pragma unroll
                    for (int k = 0; k < 4; k++) cell[j][k] += x[j][k] > u ? 1u : 0u;
            }
        }
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int f = f0 + 8 * j;
            // a value staged as 0 (node >= N, frame >= B) may count thresholds below 0: its rows are never stored, its frames masked
            tile[tile_at<PACK>(f, c)] = cell[j][0] | (cell[j][1] << 8) | (cell[j][2] << 16) | (cell[j][3] << 24);
        }
    }
    __syncthreads();
    const int lane = t & 63;
    const uint32_t cha_w = reinterpret_cast<const uint32_t *>(tab->lut_cha)[lane], msg_w = reinterpret_cast<const uint32_t *>(tab->lut_msg)[lane];
    uint32_t live[PACK];
    live_frames<PACK>(live, g, lane, B);
    rows_from_tile<PACK, 0, 1>(tile, g, n0, N, dst_cha, dst_msg,
                               [&](uint32_t x, int h) { return wave_lut4(cha_w, x) & live[h]; },
                               [&](uint32_t x, int h) { return wave_lut4(msg_w, x) & live[h]; });
}

}  // namespace lutldpc
