// decoder_llr.hip -- the two batch decodes on soft values, one quantiser: lutldpc_decoder_decode_llr_packed for receivers, whose
// values are float32, float16 or 8-bit fixed point and sit in host memory or already on the device, and
// lutldpc_decoder_decode_llr_batch, the toolkit's own float64 entry (host memory, a byte per decided bit back).  Values -> cells ->
// both row sets in one pass (llr_cells.hpp, kernels_llr.hpp) -> decode_tiles -> packed bits (bits_to_caller) or bytes
// (rows_to_host); every decode path decode_tiles picks.  Home of the kernel of kernels_llr.hpp; lutldpc_llr_cell_table is the
// host half on its own.
#include "decoder_state.hpp"
#include "kernels_llr.hpp"
#include "llr_cells.hpp"

#pragma GCC visibility push(hidden)

// (see preload_code_objects) this unit's code object
hipError_t preload_llr_kernels() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&llr_labels_in_kernel<2, float, 1>));
}

// frame-major values of B frames (device, `stride` elements per frame) -> d_cha_t / d_msg0_t
template <class T>
static int launch_llr_labels_in(lutldpc_decoder *d, const void *src, size_t stride, const LlrTables *tab, int n_thr, int B, int G) {
    const dim3 grid((unsigned)((d->nvar + 127) / 128), (unsigned)G);
    const T *p = static_cast<const T *>(src);
    const bool vec = stride % 4 == 0 && reinterpret_cast<uintptr_t>(src) % alignof(LlrQuad<T>) == 0;
#define LLR_IN(VEC) PACK_DISPATCH(d, launch_k(llr_labels_in_kernel<PK, T, VEC>, grid, dim3(256), 0, d->stream, p, stride, d->d_cha_t.p, d->d_msg0_t.p, tab, n_thr, B, d->nvar))
    if (vec) LLR_IN(1); else LLR_IN(0);
#undef LLR_IN
    LAUNCH_CHECK();
    return LUTLDPC_OK;
}

// the tables of a call as the kernel of `dtype` reads them
static LlrTables device_tables(const LlrCells &C, int dtype) {
    LlrTables T;
    memset(&T, 0, sizeof(T));                               // (the arena is keyed by content: no stray bytes)
    memcpy(T.lut_cha, C.lut_cha, 256);
    memcpy(T.lut_msg, C.lut_msg, 256);
    for (int j = 0; j < C.n_thr; j++) {
        if (dtype == LUTLDPC_LLR_F64) T.thr.f64[j] = C.thr[j];
        else T.thr.f32[j] = (float)C.thr[j];                // exact: a value of float32 / float16
    }
    return T;
}

// The values of B frames as io describes them (element type, host or device memory, frame stride) through the cells C of that io
// into both row sets: host values staged as they came (the whole batch, gaps included, up to the last element read), one kernel.
static int llr_rows_in(lutldpc_decoder *d, const lutldpc_llr_io &io, const LlrCells &C, const void *llr, int B) {
    int rc;
    const size_t stride = io.frame_stride ? (size_t)io.frame_stride : (size_t)d->nvar;
    const void *src = llr;
    if (!io.on_device) {
        const size_t bytes = ((size_t)(B - 1) * stride + (size_t)d->nvar) * llr_elem_size(io.dtype);
        HIP_TRY(d->d_host_in.alloc((bytes + 7) / 8));
        HIP_TRY(hipMemcpyAsync(d->d_host_in.p, llr, bytes, hipMemcpyHostToDevice, d->stream));
        src = d->d_host_in.p;
    }
    if ((rc = ensure_batch(d, B))) return rc;
    const int G = d->bpad(B) / d->tile();
    Timed t(d, LUTLDPC_K_LAYOUT);
    DEV_PARAM(tab, d, device_tables(C, io.dtype));
    switch (io.dtype) {
    case LUTLDPC_LLR_F64: return launch_llr_labels_in<double>(d, src, stride, tab, C.n_thr, B, G);
    case LUTLDPC_LLR_F32: return launch_llr_labels_in<float>(d, src, stride, tab, C.n_thr, B, G);
    case LUTLDPC_LLR_F16: return launch_llr_labels_in<_Float16>(d, src, stride, tab, C.n_thr, B, G);
    default: return launch_llr_labels_in<int8_t>(d, src, stride, tab, C.n_thr, B, G);
    }
}

#pragma GCC visibility pop

extern "C" int lutldpc_llr_cell_table(const lutldpc_llr_io *io, int Nq_Cha, int Nq_Msg0, double *thr, int32_t thr_cap, int32_t *n_thr,
                                      uint8_t lut_cha[256], uint8_t lut_msg[256]) {
    if (!io || !n_thr || !lut_cha || !lut_msg) return fail(LUTLDPC_ERR_ARG, "NULL argument");
    LlrCells C;
    const std::string err = llr_cell_table(*io, Nq_Cha, Nq_Msg0, C);
    if (!err.empty()) return fail(LUTLDPC_ERR_ARG, err);
    if (C.n_thr > thr_cap || (C.n_thr > 0 && !thr)) return fail(LUTLDPC_ERR_ARG, "thr holds fewer than " + std::to_string(C.n_thr) + " thresholds");
    *n_thr = C.n_thr;
    std::copy(C.thr, C.thr + C.n_thr, thr);
    memcpy(lut_cha, C.lut_cha, 256);
    memcpy(lut_msg, C.lut_msg, 256);
    return LUTLDPC_OK;
}

extern "C" int lutldpc_decoder_decode_llr_packed(lutldpc_decoder *d, const lutldpc_llr_io *io, const void *llr, int B, uint32_t *out_words,
                                                 int32_t *out_iters, uint8_t *out_cha, uint8_t *out_msg0) {
    if (!d) return fail(LUTLDPC_ERR_ARG, "NULL decoder");
    if (B <= 0) return fail(LUTLDPC_ERR_ARG, "B must be positive");
    if (!io || !llr) return fail(LUTLDPC_ERR_ARG, "NULL argument: io and llr are required");
    const size_t esize = llr_elem_size(io->dtype);
    if (!esize) return fail(LUTLDPC_ERR_ARG, "dtype must be LUTLDPC_LLR_F64, _F32, _F16 or _I8");
    if (reinterpret_cast<uintptr_t>(llr) % esize) return fail(LUTLDPC_ERR_ARG, "llr is not aligned to its element size");
    const int N = d->nvar;
    if (io->frame_stride != 0 && io->frame_stride < N) return fail(LUTLDPC_ERR_ARG, "frame_stride must be 0 or at least nvar");
    LlrCells C;
    const std::string err = llr_cell_table(*io, d->Nq_Cha, d->Nq_Msg[0], C);
    if (!err.empty()) return fail(LUTLDPC_ERR_ARG, err);
    int rc = out_words ? check_out_window(d, io->out_first, io->out_count) : LUTLDPC_OK;
    if (rc) return rc;
    if (!out_words && !out_iters && !out_cha && !out_msg0) return fail(LUTLDPC_ERR_ARG, "no output asked for");
    if ((rc = batch_entry(d, B))) return rc;
    const bool dev = io->on_device != 0, decode = out_words || out_iters;
    if ((rc = llr_rows_in(d, *io, C, llr, B))) return rc;
    const int G = d->bpad(B) / d->tile();
    // the labels the device derived, read back from the rows before the decode works on them
    const uint8_t *rows[2] = {d->d_cha_t.p, d->d_msg0_t.p};
    uint8_t *labels[2] = {out_cha, out_msg0};
    for (int i = 0; i < 2; i++) {
        if (!labels[i]) continue;
        if (!dev) { if ((rc = rows_to_host(d, rows[i], labels[i], B))) return rc; continue; }
        Timed t(d, LUTLDPC_K_LAYOUT);
        if ((rc = launch_transpose_out(d, rows[i], labels[i], B, G))) return rc;
    }
    if (decode && (rc = decode_tiles(d, B))) return rc;
    if (out_words && (rc = bits_to_caller(d, out_words, dev, B, io->out_first, io->out_count))) return rc;
    if (out_iters) {
        if (dev) HIP_TRY(hipMemcpyAsync(out_iters, d->d_iters.p, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToDevice, d->stream));
        else if ((rc = iters_to_host(d, out_iters, B))) return rc;
    }
    if (!dev || io->sync) HIP_TRY(hipStreamSynchronize(d->stream));
    return LUTLDPC_OK;
}

// The float64 entry takes the boundary arrays its callers hold, sorted or not: quant_nonlin's leading count on any array
// (leading_count_bounds).  Mode 0 ignores a given map, mode 1 ignores qb_Msg / n_qb_Msg.  A cha2msg_map entry outside
// [0, Nq_Msg[0]) in mode 1 is LUTLDPC_ERR_ARG (llr_cell_table): no row may hold a label outside its alphabet.
extern "C" int lutldpc_decoder_decode_llr_batch(lutldpc_decoder *d, const double *llr, int B, const double *qb_Cha, int n_qb_Cha,
                                                const double *qb_Msg, int n_qb_Msg, int mode, const int32_t *map,
                                                uint8_t *out_bits, int32_t *out_iters) {
    if (!d || !llr || !qb_Cha || !out_bits || !out_iters) return fail(LUTLDPC_ERR_ARG, "NULL argument");
    int rc = batch_entry(d, B);
    if (rc) return rc;
    if (n_qb_Cha != d->Nq_Cha - 1) return fail(LUTLDPC_ERR_ARG, "qb_Cha must hold Nq_Cha-1 boundaries");
    if (mode == 0 && (!qb_Msg || n_qb_Msg != d->Nq_Msg[0] - 1)) return fail(LUTLDPC_ERR_ARG, "qb_Msg must hold Nq_Msg[0]-1 boundaries");
    if (mode == 1 && !map) return fail(LUTLDPC_ERR_ARG, "QCHA mode needs cha2msg_map");
    if (mode != 0 && mode != 1) return fail(LUTLDPC_ERR_ARG, "initial_message_mode must be 0 (CONT) or 1 (QCHA)");   // src/LDPC_Code_LUT.cpp:218-220
    const std::vector<double> cha = leading_count_bounds(qb_Cha, n_qb_Cha), msg = leading_count_bounds(qb_Msg, mode == 0 ? n_qb_Msg : 0);
    lutldpc_llr_io io{};                                    // host memory
    io.dtype = LUTLDPC_LLR_F64; io.frame_stride = d->nvar;
    io.qb_Cha = cha.data(); io.n_qb_Cha = n_qb_Cha;
    if (mode == 0) { io.qb_Msg = msg.data(); io.n_qb_Msg = n_qb_Msg; }
    else io.cha2msg_map = map;
    io.initial_message_mode = mode;
    LlrCells C;
    const std::string err = llr_cell_table(io, d->Nq_Cha, d->Nq_Msg[0], C);
    if (!err.empty()) return fail(LUTLDPC_ERR_ARG, err);
    if ((rc = llr_rows_in(d, io, C, llr, B)) || (rc = decode_tiles(d, B)) ||
        (rc = rows_to_host(d, d->d_hard.p, out_bits, B)) || (rc = iters_to_host(d, out_iters, B))) return rc;
    HIP_TRY(hipStreamSynchronize(d->stream));
    return LUTLDPC_OK;
}
