// decoder_layout.hip -- host launchers of the kernels that move a batch between the caller's frame-major form and the row layout:
// labels in (bytes or nibbles, one or two row sets), labels out (any row set, the message trace included) and decided bits out.
// Home of every kernel of kernels_layout.hpp.
#include "decoder_state.hpp"
#include "kernels_layout.hpp"

#pragma GCC visibility push(hidden)

// (see preload_code_objects) this unit's code object
hipError_t preload_layout_kernels() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&labels_in_kernel<2, 0, 1, 0>));
}

// The dword-vectorised forms need a frame size that is a multiple of 4 bytes and a 4-byte aligned frame-major buffer.
int launch_labels_in(lutldpc_decoder *d, const uint8_t *src, size_t stride, bool nibbles, uint8_t *rows_a, uint8_t *rows_b, const uint8_t *lut_b,
                     int B, int G, int lim_a) {
    const dim3 grid((unsigned)((stride + 127) / 128), (unsigned)G);
    const bool vec = stride % 4 == 0 && (reinterpret_cast<uintptr_t>(src) & 3u) == 0;
#define LABELS_IN(NIB, VEC, TWO) PACK_DISPATCH(d, launch_k(labels_in_kernel<PK, NIB, VEC, TWO>, grid, dim3(256), 0, d->stream, src, (int)stride, rows_a, rows_b, lut_b, B, d->nvar, lim_a))
#define LABELS_IN_ROWS(NIB, VEC) do { if (rows_b) LABELS_IN(NIB, VEC, 1); else LABELS_IN(NIB, VEC, 0); } while (0)
    if (nibbles) { if (vec) LABELS_IN_ROWS(1, 1); else LABELS_IN_ROWS(1, 0); }
    else { if (vec) LABELS_IN_ROWS(0, 1); else LABELS_IN_ROWS(0, 0); }
#undef LABELS_IN_ROWS
#undef LABELS_IN
    LAUNCH_CHECK();
    return LUTLDPC_OK;
}

int launch_transpose_out(lutldpc_decoder *d, const uint8_t *src_rows, uint8_t *dst, int B, int G, int rows) {
    const int N = rows > 0 ? rows : d->nvar;
    const dim3 grid((unsigned)((N + 127) / 128), (unsigned)G);
    if (N % 4 == 0 && (reinterpret_cast<uintptr_t>(dst) & 3u) == 0)
        PACK_DISPATCH(d, launch_k(transpose_out_kernel<PK, 1>, grid, dim3(256), 0, d->stream, src_rows, dst, B, N));
    else
        PACK_DISPATCH(d, launch_k(transpose_out_kernel<PK, 0>, grid, dim3(256), 0, d->stream, src_rows, dst, B, N));
    LAUNCH_CHECK();
    return LUTLDPC_OK;
}

int launch_bits_out(lutldpc_decoder *d, uint32_t *dst, int B, int G, int first, int count) {
    const int W = (count + 31) / 32;
    PACK_DISPATCH(d, launch_k(packed_bits_out_kernel<PK>, dim3((unsigned)((W + kBitsCols - 1) / kBitsCols), (unsigned)G), dim3(256), 0, d->stream,
                              d->d_hard.p, dst, B, d->nvar, first, count, W));
    LAUNCH_CHECK();
    return LUTLDPC_OK;
}

#pragma GCC visibility pop
