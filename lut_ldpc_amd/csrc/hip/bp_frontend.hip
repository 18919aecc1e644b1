// bp_frontend.hip -- the device front end of the [BP] comparison decoder (C-ABI and specification: include/lut_ldpc_bp.h; kernels:
// kernels_bp_frontend.hpp): lutldpc_bp_set_cells, lutldpc_bp_sample_qllr, lutldpc_bp_sim_batch.
//
// The body of the frame loop of LDPC_BER_Sim::sim_snr_point (src/LDPC_BER_Sim.cpp:262-286) for a batch of frames without a host
// round trip: sampler -> d_in rows -> bp_decode (bp_decoder.hip) -> d_out rows -> counters; 16 bytes per frame come back.
#include "bp_state.hpp"
#include "kernels_bp_frontend.hpp"

#include <algorithm>

using namespace lutldpc_bp;

namespace {

constexpr int kMaxBatch = 1 << 28;     // 4 B counters and Bpad = B rounded up to 256 stay ints

// the guards the two batch entries share, in the order the header states (mandatory pointers are checked by the caller in between)
int entry_args(const lutldpc_bp_decoder *d, int B) {
    if (!d) return bp_fail(LUTLDPC_ERR_ARG, "NULL decoder");
    if (B <= 0 || B > kMaxBatch) return bp_fail(LUTLDPC_ERR_ARG, "B must be in 1 .. 2^28");
    return LUTLDPC_OK;
}
int entry_state(const lutldpc_bp_decoder *d, uint32_t stream) {
    if (int rc = lutldpc_check_stream(stream)) return rc;
    if (d->device < 0) return bp_fail(LUTLDPC_ERR_STATE, "BP decoder was created without a device (host-only handle)");
    if (d->n_cells <= 0) return bp_fail(LUTLDPC_ERR_STATE, "no cell table set (lutldpc_bp_set_cells)");
    return LUTLDPC_OK;
}

unsigned chunk_blocks(int nodes) { return (unsigned)std::max(1, std::min((nodes + lutldpc::kBpChunkNodes - 1) / lutldpc::kBpChunkNodes, 2048)); }

// sent bits to the device, rows allocated, sampler enqueued: d_in and d_unc hold the batch
int sample_rows(lutldpc_bp_decoder *d, uint64_t seed, uint32_t stream, uint64_t frame0, int B, int Bpad, const uint8_t *codewords) {
    BP_TRY(hipSetDevice(d->device));
    if (int rc = alloc_rows(d, Bpad)) return rc;
    BP_TRY(d->d_unc.alloc((size_t)Bpad));
    const size_t n = (size_t)B * d->nvar;
    if (codewords) {
        BP_TRY(d->d_cw.alloc(n));
        BP_TRY(hipMemcpyAsync(d->d_cw.p, codewords, n, hipMemcpyHostToDevice, d->stream));
    }
    const dim3 grid(chunk_blocks(d->nvar), (unsigned)(Bpad / 256));
    lutldpc::launch_k(lutldpc::bp_zero_kernel, dim3((unsigned)(Bpad / 256)), dim3(256), 0, d->stream, d->d_unc.p, Bpad);
    if (codewords)
        lutldpc::launch_k(lutldpc::bp_sample_qllr_kernel<true>, grid, dim3(256), 0, d->stream, d->d_thr.p, d->d_attr.p, d->d_first.p, (uint32_t)seed, (uint32_t)(seed >> 32),
                          stream, frame0, B, d->nvar, Bpad, d->d_cw.p, d->d_in.p, d->d_unc.p);
    else
        lutldpc::launch_k(lutldpc::bp_sample_qllr_kernel<false>, grid, dim3(256), 0, d->stream, d->d_thr.p, d->d_attr.p, d->d_first.p, (uint32_t)seed, (uint32_t)(seed >> 32),
                          stream, frame0, B, d->nvar, Bpad, (const uint8_t *)nullptr, d->d_in.p, d->d_unc.p);
    return LUTLDPC_OK;
}

int launch_error() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? LUTLDPC_OK : bp_fail(LUTLDPC_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
}

}  // namespace

extern "C" {

int lutldpc_bp_set_cells(lutldpc_bp_decoder *d, const lutldpc_bp_cells *cells) {
    if (!d || !cells || !cells->thr || !cells->qllr || !cells->slicer_neg) return bp_fail(LUTLDPC_ERR_ARG, "NULL decoder, table or member of the table");
    const int n = cells->n_cells;
    if (n < 1 || n > LUTLDPC_BP_MAX_CELLS) return bp_fail(LUTLDPC_ERR_ARG, "n_cells must be in 1 .. " + std::to_string(LUTLDPC_BP_MAX_CELLS));
    for (int j = 1; j < n - 1; j++)
        if (cells->thr[j] < cells->thr[j - 1]) return bp_fail(LUTLDPC_ERR_ARG, "thresholds descend at cell " + std::to_string(j));
    for (int j = 0; j < n; j++)
        if (cells->qllr[j] > d->qmax || cells->qllr[j] < -d->qmax) return bp_fail(LUTLDPC_ERR_ARG, "|qllr| above QMAX at cell " + std::to_string(j));
    if (d->device < 0) return bp_fail(LUTLDPC_ERR_STATE, "BP decoder was created without a device (host-only handle)");
    // the slice index: first[s] = thresholds <= s << (64 - kBpSliceBits), by one merge over the ascending thresholds
    constexpr int S = 1 << lutldpc::kBpSliceBits;
    std::vector<uint64_t> thr(cells->thr, cells->thr + (n - 1));
    std::vector<int32_t> attr((size_t)n);
    std::vector<uint32_t> first((size_t)S + 1);
    for (int j = 0; j < n; j++) attr[(size_t)j] = cells->qllr[j] * 2 + (cells->slicer_neg[j] ? 1 : 0);     // |q| <= QMAX < 2^28
    lutldpc::slice_index<lutldpc::kBpSliceBits>(thr.data(), n - 1, first.data());
    first[(size_t)S] = (uint32_t)(n - 1);
    BP_TRY(hipSetDevice(d->device));
    BP_TRY(hipStreamSynchronize(d->stream));       // no batch of the previous table is in flight (before the uploads: nothing to release if it fails)
    Buf<uint64_t> n_thr; Buf<int32_t> n_attr; Buf<uint32_t> n_first;
    const hipError_t e1 = n_thr.upload(thr), e2 = e1 == hipSuccess ? n_attr.upload(attr) : e1, e3 = e2 == hipSuccess ? n_first.upload(first) : e2;
    if (e3 != hipSuccess) {
        n_thr.release(); n_attr.release(); n_first.release();
        return bp_fail(LUTLDPC_ERR_HIP, std::string("cell table upload: ") + hipGetErrorString(e3));
    }
    d->d_thr.swap(n_thr); d->d_attr.swap(n_attr); d->d_first.swap(n_first);
    n_thr.release(); n_attr.release(); n_first.release();
    d->n_cells = n;
    return LUTLDPC_OK;
}

int lutldpc_bp_sample_qllr(lutldpc_bp_decoder *d, uint64_t seed, uint32_t stream, uint64_t frame0, int B, const uint8_t *codewords, int32_t *qllr_out,
                           int32_t *uncoded_out) {
    if (int rc = entry_args(d, B)) return rc;
    if (!qllr_out) return bp_fail(LUTLDPC_ERR_ARG, "qllr_out is NULL");
    if (int rc = entry_state(d, stream)) return rc;
    const int Bpad = (B + 255) / 256 * 256;
    const size_t n = (size_t)B * d->nvar;
    if (int rc = sample_rows(d, seed, stream, frame0, B, Bpad, codewords)) return rc;
    BP_TRY(d->d_q_out.alloc(n));
    store_rows(d, d->d_in.p, nullptr, d->d_q_out.p, B, Bpad);
    if (int rc = launch_error()) return rc;
    BP_TRY(hipMemcpyAsync(qllr_out, d->d_q_out.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, d->stream));
    if (uncoded_out) BP_TRY(hipMemcpyAsync(uncoded_out, d->d_unc.p, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, d->stream));
    BP_TRY(hipStreamSynchronize(d->stream));
    return LUTLDPC_OK;
}

int lutldpc_bp_sim_batch(lutldpc_bp_decoder *d, uint64_t seed, uint32_t stream, uint64_t frame0, int B, const uint8_t *codewords, int K_info,
                         int32_t *frame_stats, int32_t *qllr_out, uint8_t *bits_out) {
    if (int rc = entry_args(d, B)) return rc;
    if (!frame_stats) return bp_fail(LUTLDPC_ERR_ARG, "frame_stats is NULL");
    if (K_info < 0 || K_info > d->nvar) return bp_fail(LUTLDPC_ERR_ARG, "K_info must be in 0 .. nvar");
    if (int rc = entry_state(d, stream)) return rc;
    const int Bpad = (B + 255) / 256 * 256;
    const size_t n = (size_t)B * d->nvar;
    if (int rc = sample_rows(d, seed, stream, frame0, B, Bpad, codewords)) return rc;
    BP_TRY(d->d_stats.alloc((size_t)B * 4));
    if (qllr_out) BP_TRY(d->d_q_out.alloc(n));
    if (bits_out) BP_TRY(d->d_bits.alloc(n));
    if (qllr_out) {                                 // the decoder's input, before the decode (one staging buffer, copies are stream-ordered)
        store_rows(d, d->d_in.p, nullptr, d->d_q_out.p, B, Bpad);
        BP_TRY(hipMemcpyAsync(qllr_out, d->d_q_out.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, d->stream));
    }
    if (int rc = decode_rows(d, B, Bpad)) return rc;
    lutldpc::launch_k(lutldpc::bp_zero_kernel, dim3((unsigned)((B * 4 + 255) / 256)), dim3(256), 0, d->stream, d->d_stats.p, B * 4);
    const dim3 grid(chunk_blocks(K_info), (unsigned)(Bpad / 256));
    if (codewords)
        lutldpc::launch_k(lutldpc::bp_count_errors_kernel<true>, grid, dim3(256), 0, d->stream, d->d_out.p, d->d_cw.p, d->d_iters.p, d->d_unc.p, B, d->nvar, K_info, Bpad, d->d_stats.p);
    else
        lutldpc::launch_k(lutldpc::bp_count_errors_kernel<false>, grid, dim3(256), 0, d->stream, d->d_out.p, (const uint8_t *)nullptr, d->d_iters.p, d->d_unc.p, B, d->nvar, K_info, Bpad,
                          d->d_stats.p);
    if (bits_out) store_rows(d, d->d_out.p, d->d_bits.p, nullptr, B, Bpad);
    if (int rc = launch_error()) return rc;
    BP_TRY(hipMemcpyAsync(frame_stats, d->d_stats.p, sizeof(int32_t) * 4 * (size_t)B, hipMemcpyDeviceToHost, d->stream));
    if (bits_out) BP_TRY(hipMemcpyAsync(bits_out, d->d_bits.p, n, hipMemcpyDeviceToHost, d->stream));
    BP_TRY(hipStreamSynchronize(d->stream));
    return LUTLDPC_OK;
}

}  // extern "C"
