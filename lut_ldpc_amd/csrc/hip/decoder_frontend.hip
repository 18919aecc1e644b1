// decoder_frontend.hip -- the simulation front end on the device: channel sampler, random-codeword encoder, error counters, the
// encoder of the caller's packed data bits, and the C-ABI entries built on them.  Home of every kernel of kernels_frontend.hpp,
// kernels_encode.hpp and kernels_encode_sparse.hpp.
#include "decoder_state.hpp"
#include "kernels_frontend.hpp"
#include "kernels_encode.hpp"
#include "kernels_encode_sparse.hpp"
#include "../host/sparse_generator.hpp"

static_assert(kSparseBlockRows == lut_ldpc::kSparseBlock, "the block of the host's inverse rows is the block of sparse_phase_b_kernel");

#pragma GCC visibility push(hidden)

// (see preload_code_objects) this unit's code object
hipError_t preload_frontend_kernels() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&encode_random_kernel));
}

int fill_cells(const lutldpc_channel_cells *c, const lutldpc_decoder *d, ChannelCells &C) {
    if (!c || !c->thr || !c->cha_label || !c->msg_label || !c->slicer_neg || !c->cha_label_mirror || !c->msg_label_mirror)
        return fail(LUTLDPC_ERR_ARG, "channel cells: NULL member");
    if (c->n_cells < 1 || c->n_cells > kMaxCells) return fail(LUTLDPC_ERR_ARG, "channel cells: n_cells outside [1,72]");
    std::memset(&C, 0, sizeof(C));
    C.n_cells = c->n_cells;
    for (int j = 0; j < c->n_cells; j++) {
        if (j < c->n_cells - 1) { C.thr[j] = c->thr[j]; if (j && c->thr[j] < c->thr[j - 1]) return fail(LUTLDPC_ERR_ARG, "channel cells: thresholds must ascend"); }
        if (c->cha_label[j] >= d->Nq_Cha || c->cha_label_mirror[j] >= d->Nq_Cha || c->msg_label[j] >= d->Nq_Msg[0] || c->msg_label_mirror[j] >= d->Nq_Msg[0])
            return fail(LUTLDPC_ERR_ARG, "channel cells: label outside its alphabet");
        C.cha[j] = c->cha_label[j]; C.msg[j] = c->msg_label[j]; C.neg[j] = c->slicer_neg[j] ? 1 : 0;
        C.cha_m[j] = c->cha_label_mirror[j]; C.msg_m[j] = c->msg_label_mirror[j];
    }
    return LUTLDPC_OK;
}

// sampler -> d_cha_t / d_msg0_t (tile layout); stats zeroed and slicer errors accumulated.  sent_rows: the sent bits of the
// batch (sent_rows_of), null = all-zero codeword
int sample_tiles(lutldpc_decoder *d, const ChannelCells &C, uint64_t seed, uint32_t stream, uint64_t frame0, int B, const uint8_t *sent_rows) {
    int rc = ensure_batch(d, B);
    if (rc) return rc;
    const int Bpad = d->bpad(B), G = Bpad / d->tile(), N = d->nvar;
    HIP_TRY(d->d_stats.alloc((size_t)Bpad * 4));
    HIP_TRY(hipMemsetAsync(d->d_stats.p, 0, sizeof(int32_t) * (size_t)Bpad * 4, d->stream));
    Timed t(d, LUTLDPC_K_FRONTEND);
    const int ppt = 8, npairs = (N + 1) / 2;
    dim3 grid((unsigned)((npairs + 4 * ppt - 1) / (4 * ppt)), (unsigned)G);
    DEV_PARAM(dC, d, C);
    if (sent_rows)
        PACK_DISPATCH(d, launch_k(sample_labels_kernel<PK, true>, grid, dim3(256), 0, d->stream, dC, (uint32_t)seed, (uint32_t)(seed >> 32), stream, frame0, B, N,
                           sent_rows, d->d_cha_t.p, d->d_msg0_t.p, d->d_stats.p, ppt));
    else
        PACK_DISPATCH(d, launch_k(sample_labels_kernel<PK>, grid, dim3(256), 0, d->stream, dC, (uint32_t)seed, (uint32_t)(seed >> 32), stream, frame0, B, N,
                           sent_rows, d->d_cha_t.p, d->d_msg0_t.p, d->d_stats.p, ppt));
    LAUNCH_CHECK();
    return LUTLDPC_OK;
}

// The sparse form: the parity rows K .. K+R-1 of `rows` (G frame groups, information rows in place) from the information rows --
// phase A (s = A u) and phase B (p = T^-1 s, in place), ordered by the stream
static int launch_sparse_parity(lutldpc_decoder *d, uint8_t *rows, int G) {
    const int K = d->gen_K, R = d->gen_R, N = d->nvar, DW = d->tile() / 32;
    if (R < 1) return LUTLDPC_OK;
    uint32_t *r32 = reinterpret_cast<uint32_t *>(rows);
    const int gpw = 64 / DW;                    // frame groups per wave of phase A
    launch_k(sparse_phase_a_kernel, dim3((unsigned)((R + 3) / 4), (unsigned)((G + gpw - 1) / gpw)), dim3(256), 0, d->stream, d->sp.a_ptr.p, d->sp.a_cols.p, K, R, N, G, DW, r32);
    LAUNCH_CHECK();
    launch_k(sparse_phase_b_kernel, dim3((unsigned)(G * (DW / kSparseSliceDwords))), dim3(256), 0, d->stream, d->sp.order.p, d->sp.e_ptr.p, d->sp.e_cols.p, d->sp.inv.p,
             K, d->sp.Rp, N, DW, r32);
    LAUNCH_CHECK();
    return LUTLDPC_OK;
}

// random codewords of frames frame0 .. frame0+B-1 -> d_sent (sent-bit rows of bpad(B) frames; pad frames zero)
int encode_tiles(lutldpc_decoder *d, uint64_t seed, uint32_t stream, uint64_t frame0, int B) {
    if (!d->gen_set) return fail(LUTLDPC_ERR_STATE, "no generator set: random codewords on the device need lutldpc_decoder_set_generator first");
    const int Bpad = d->bpad(B), G = Bpad / d->tile(), N = d->nvar;
    const int RB = d->pack == 2 ? sent_row_bytes<2>() : sent_row_bytes<1>();
    HIP_TRY(d->d_sent.alloc((size_t)G * N * RB));
    Timed t(d, LUTLDPC_K_FRONTEND);
    const int K = d->gen_K, R = d->gen_R;
    if (d->gen_sparse) {
        const unsigned ny = (unsigned)std::min(64, std::max(1, ((K + 127) / 128 + 3) / 4));
        launch_k(info_rows_random_kernel, dim3((unsigned)(Bpad / 64), ny), dim3(256), 0, d->stream, K, (uint32_t)seed, (uint32_t)(seed >> 32), stream, frame0, B, N,
                 d->tile(), d->d_sent.p);
        LAUNCH_CHECK();
        return launch_sparse_parity(d, d->d_sent.p, G);
    }
    const int W128 = (K + 127) / 128, T = (R + kEncTileRows - 1) / kEncTileRows, W32 = (K + 31) / 32;
    // one wave per parity tile (at least one information word per wave where the tiles are fewer); a workgroup is 64 frames
    const unsigned gx = (unsigned)(Bpad / kEncFrames), gy = (unsigned)std::max(1, (std::max(T, (W32 + 7) / 8) + 3) / 4);
    launch_k(encode_random_kernel, dim3(gx, gy), dim3(256), (size_t)W128 * kEncFrames * 16, d->stream, d->d_gen.p, K, R, d->gen_W32p,
             (uint32_t)seed, (uint32_t)(seed >> 32), stream, frame0, B, N, d->tile(), d->d_sent.p);
    LAUNCH_CHECK();
    return LUTLDPC_OK;
}

// d_sent -> frame-major bytes at dst (device, B*N)
static int launch_sent_to_bytes(lutldpc_decoder *d, uint8_t *dst, int B) {
    const size_t n = (size_t)B * d->nvar;
    PACK_DISPATCH(d, launch_k(sent_rows_to_bytes_kernel<PK>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, d->stream, d->d_sent.p, B, d->nvar, dst));
    LAUNCH_CHECK();
    return LUTLDPC_OK;
}

// The one device form of the sent bits of a batch: sent-bit rows in d_sent -- made by the encoder from (seed, stream, frame)
// (device_codewords), or converted once from the caller's frame-major bytes (codewords, host) -- or *rows = null: the all-zero
// codeword.  Sampler, error counters, histograms and the capture all read this.
int sent_rows_of(lutldpc_decoder *d, const uint8_t *codewords, bool device_codewords, uint64_t seed, uint32_t stream, uint64_t frame0, int B,
                 const uint8_t **rows) {
    if (!device_codewords) return sent_rows_from_host(d, codewords, B, rows);
    const int rc = encode_tiles(d, seed, stream, frame0, B);
    *rows = d->d_sent.p;
    return rc;
}

// lutldpc_decoder_sim_batch (codewords: host, frame-major, or null) and lutldpc_decoder_sim_batch_random (device_codewords:
// made by the encoder on the device from (seed, stream, frame))
int sim_batch_impl(lutldpc_decoder *d, const lutldpc_channel_cells *cells, uint64_t seed, uint32_t stream, uint64_t frame0, int B,
                   const uint8_t *codewords, bool device_codewords, int K_info, int32_t *frame_stats, uint8_t *cha_out, uint8_t *bits_out, lutldpc_event_request *req) {
    if (!d || !frame_stats) return fail(LUTLDPC_ERR_ARG, "NULL argument");
    int rc = batch_entry(d, B, stream);
    if (rc) return rc;
    if (K_info < 0 || K_info > d->nvar) return fail(LUTLDPC_ERR_ARG, "bad K_info");
    if (device_codewords && !d->gen_set) return fail(LUTLDPC_ERR_STATE, "sim_batch_random: no generator set (lutldpc_decoder_set_generator)");
    ChannelCells C;
    if ((rc = fill_cells(cells, d, C))) return rc;
    const uint8_t *sent_rows = nullptr;
    if ((rc = sent_rows_of(d, codewords, device_codewords, seed, stream, frame0, B, &sent_rows))) return rc;
    if ((rc = sample_tiles(d, C, seed, stream, frame0, B, sent_rows))) return rc;
    // the sampled labels, read back from the rows before the decode works on them: a decode that compacts leaves the channel rows
    // in slot order (launch_uncompaction brings back the decided bits and the iteration codes only)
    if (cha_out && (rc = rows_to_host(d, d->d_cha_t.p, cha_out, B))) return rc;
    if ((rc = decode_tiles(d, B))) return rc;
    {
        Timed t(d, LUTLDPC_K_FRONTEND);
        const int Bpad = d->bpad(B), G = Bpad / d->tile(), rpw = 64;
        const int rows = K_info > 0 ? K_info : 1;
        const dim3 grid((unsigned)((rows + 4 * rpw - 1) / (4 * rpw)), (unsigned)G);
        if (sent_rows)
            PACK_DISPATCH(d, launch_k(count_errors_kernel<PK, true>, grid, dim3(256), 0, d->stream, d->d_hard.p, sent_rows, B, d->nvar, K_info, d->d_iters.p, d->d_stats.p, rpw));
        else
            PACK_DISPATCH(d, launch_k(count_errors_kernel<PK>, grid, dim3(256), 0, d->stream, d->d_hard.p, sent_rows, B, d->nvar, K_info, d->d_iters.p, d->d_stats.p, rpw));
        LAUNCH_CHECK();
    }
    if ((rc = copy_to_host(d, frame_stats, d->d_stats.p, sizeof(int32_t) * (size_t)B * 4))) return rc;
    if (bits_out && (rc = rows_to_host(d, d->d_hard.p, bits_out, B))) return rc;
    if (req && (rc = capture_events(d, B, K_info, sent_rows, d->d_stats.p, req))) return rc;
    HIP_TRY(hipStreamSynchronize(d->stream));
    return LUTLDPC_OK;
}

#pragma GCC visibility pop

extern "C" {

int lutldpc_decoder_sim_batch(lutldpc_decoder *d, const lutldpc_channel_cells *cells, uint64_t seed, uint32_t stream, uint64_t frame0, int B,
                              const uint8_t *codewords, int K_info, int32_t *frame_stats, uint8_t *cha_out, uint8_t *bits_out) {
    return sim_batch_impl(d, cells, seed, stream, frame0, B, codewords, false, K_info, frame_stats, cha_out, bits_out);
}

int lutldpc_decoder_sim_batch_random(lutldpc_decoder *d, const lutldpc_channel_cells *cells, uint64_t seed, uint32_t stream, uint64_t frame0, int B,
                                     int K_info, int32_t *frame_stats, uint8_t *cha_out, uint8_t *bits_out) {
    return sim_batch_impl(d, cells, seed, stream, frame0, B, nullptr, true, K_info, frame_stats, cha_out, bits_out);
}

int lutldpc_decoder_set_generator(lutldpc_decoder *d, int K, int R, const uint64_t *rows) {
    if (!d) return fail(LUTLDPC_ERR_ARG, "NULL decoder");
    if (!rows) return fail(LUTLDPC_ERR_ARG, "generator rows are NULL");
    if (K < 1 || R < 0 || K + R != d->nvar) return fail(LUTLDPC_ERR_ARG, "generator: K + R must equal nvar (K >= 1)");
    if (int rc = device_entry(d)) return rc;
    if (K > kEncMaxInfoBits) return fail(LUTLDPC_ERR_UNSUPPORTED, "generator: more than 8192 information bits (limit of the dense device encoder; lutldpc_decoder_set_sparse_generator has none)");
    const int WK = (K + 63) / 64, W32p = 4 * ((K + 127) / 128), Rp = (R + kEncTileRows - 1) / kEncTileRows * kEncTileRows;
    std::vector<uint32_t> a((size_t)std::max(Rp, 1) * W32p, 0u);
    for (int i = 0; i < R; i++)
        for (int j = 0; j < 2 * WK; j++) {
            const int k0 = 32 * j;
            uint32_t w = (uint32_t)(rows[(size_t)i * WK + (size_t)(j >> 1)] >> (32 * (j & 1)));
            if (k0 + 32 > K) w &= k0 >= K ? 0u : (1u << (K - k0)) - 1u;        // bits beyond K stay zero (the info words carry random bits there)
            a[(size_t)i * W32p + (size_t)j] = w;
        }
    HIP_TRY(hipStreamSynchronize(d->stream));           // (a batch in flight may still read the previous generator)
    HIP_TRY(d->d_gen.upload(a));
    d->gen_K = K; d->gen_R = R; d->gen_W32p = W32p; d->gen_set = true; d->gen_sparse = false;
    make_describe(d);
    return LUTLDPC_OK;
}

int lutldpc_decoder_set_sparse_generator(lutldpc_decoder *d, int K, int R, const int32_t *row_ptr, const int32_t *cols) {
    if (!d) return fail(LUTLDPC_ERR_ARG, "NULL decoder");
    if (!row_ptr || !cols) return fail(LUTLDPC_ERR_ARG, "sparse generator: row_ptr or cols is NULL");
    if (K < 1 || R < 0 || K + R != d->nvar) return fail(LUTLDPC_ERR_ARG, "sparse generator: K + R must equal nvar (K >= 1, R >= 0)");
    std::vector<int32_t> order;
    int depth = 0;
    const std::string bad = lut_ldpc::sparse_order(K, R, row_ptr, cols, order, depth);
    if (!bad.empty()) return fail(LUTLDPC_ERR_ARG, "sparse generator: " + bad);
    if (int rc = device_entry(d)) return rc;
    lut_ldpc::SparsePacked P;
    lut_ldpc::sparse_pack(K, R, row_ptr, cols, order, depth, P);
    const std::string oob = lut_ldpc::sparse_packed_check(P);         // every index the kernels follow, before anything reaches the device
    if (!oob.empty()) return fail(LUTLDPC_ERR_STATE, "sparse generator: packed arrays out of bounds (" + oob + ")");
    lutldpc_decoder::SparseGen up;                                     // complete before it replaces the generator in place
    HIP_TRY(up.a_ptr.upload(P.a_ptr)); HIP_TRY(up.a_cols.upload(P.a_cols)); HIP_TRY(up.order.upload(P.order));
    HIP_TRY(up.e_ptr.upload(P.e_ptr)); HIP_TRY(up.e_cols.upload(P.e_cols)); HIP_TRY(up.inv.upload(P.inv));
    up.Rp = P.Rp; up.depth = P.depth; up.terms = (long long)P.terms(); up.block = kSparseBlockRows;
    HIP_TRY(hipStreamSynchronize(d->stream));           // (a batch in flight may still read the previous generator)
    d->sp = std::move(up);
    d->gen_K = K; d->gen_R = R; d->gen_W32p = 0; d->gen_set = true; d->gen_sparse = true;
    make_describe(d);
    return LUTLDPC_OK;
}

int lutldpc_decoder_encode_random(lutldpc_decoder *d, uint64_t seed, uint32_t stream, uint64_t frame0, int B, uint8_t *codewords) {
    int rc = batch_entry(d, B, stream);
    if (rc || (rc = encode_tiles(d, seed, stream, frame0, B))) return rc;
    if (codewords) {
        const size_t n = (size_t)B * d->nvar;
        HIP_TRY(d->d_out_bits.alloc(n));
        if ((rc = launch_sent_to_bytes(d, d->d_out_bits.p, B)) || (rc = copy_to_host(d, codewords, d->d_out_bits.p, n))) return rc;
    }
    HIP_TRY(hipStreamSynchronize(d->stream));
    return LUTLDPC_OK;
}

// The caller's information bits -> codewords, bit-packed both ways, in host or device memory (encode_bits_kernel).  Works on its
// own staging buffers and the generator alone: no label rows, no frame-group state of a decode.
int lutldpc_decoder_encode_packed(lutldpc_decoder *d, const lutldpc_encode_io *io, const uint32_t *info, int B, uint32_t *out_words) {
    if (!d) return fail(LUTLDPC_ERR_ARG, "NULL decoder");
    if (B <= 0) return fail(LUTLDPC_ERR_ARG, "B must be positive");
    if (!io || !info || !out_words) return fail(LUTLDPC_ERR_ARG, "NULL argument: io, info and out_words are required");
    if (reinterpret_cast<uintptr_t>(info) % 4 || reinterpret_cast<uintptr_t>(out_words) % 4) return fail(LUTLDPC_ERR_ARG, "info and out_words must be 4-byte aligned");
    const int W32 = (d->gen_K + 31) / 32;             // (a handle without a generator: W32 = 0, and the state error below)
    if (io->in_stride < 0 || (io->in_stride != 0 && io->in_stride < W32)) return fail(LUTLDPC_ERR_ARG, "in_stride must be 0 or at least ceil(K/32)");
    int rc = check_out_window(d, io->out_first, io->out_count);
    if (rc || (rc = batch_entry(d, B))) return rc;
    if (!d->gen_set) return fail(LUTLDPC_ERR_STATE, "encode_packed: no generator set (lutldpc_decoder_set_generator)");
    const bool dev = io->on_device != 0;
    const int K = d->gen_K, R = d->gen_R, Wout = (io->out_count + 31) / 32;
    const size_t stride = io->in_stride ? (size_t)io->in_stride : (size_t)W32;
    const uint32_t *src = info;
    uint32_t *dst = out_words;
    const int G = d->bpad(B) / d->tile();
    if (d->gen_sparse) HIP_TRY(d->d_enc_rows.alloc((size_t)G * d->nvar * (size_t)(d->tile() / 8)));
    if (!dev) {         // the whole batch, gaps included, up to the last word read
        const size_t words = (size_t)(B - 1) * stride + (size_t)W32;
        HIP_TRY(d->d_llr_in.alloc((words + 1) / 2));
        HIP_TRY(hipMemcpyAsync(d->d_llr_in.p, info, words * sizeof(uint32_t), hipMemcpyHostToDevice, d->stream));
        src = reinterpret_cast<const uint32_t *>(d->d_llr_in.p);
        HIP_TRY(d->d_out_words.alloc((size_t)B * (size_t)Wout));
        dst = d->d_out_words.p;
    }
    if (d->gen_sparse) {       // bit rows of its own: information rows in, parity where the window reaches it, the window out
        Timed t(d, LUTLDPC_K_FRONTEND);
        const unsigned gx = (unsigned)(d->bpad(B) / 64);
        const unsigned ny_in = (unsigned)std::min(64, std::max(1, (W32 + 4 * kRowsWordChunk - 1) / (4 * kRowsWordChunk)));
        launch_k(info_rows_packed_kernel, dim3(gx, ny_in), dim3(256), 0, d->stream, K, src, stride, B, d->nvar, d->tile(), d->d_enc_rows.p);
        LAUNCH_CHECK();
        if (io->out_first + io->out_count > K && (rc = launch_sparse_parity(d, d->d_enc_rows.p, G))) return rc;
        const unsigned ny_out = (unsigned)std::min(64, std::max(1, (Wout + 4 * kRowsWordChunk - 1) / (4 * kRowsWordChunk)));
        launch_k(rows_window_out_kernel, dim3((unsigned)((B + 63) / 64), ny_out), dim3(256), 0, d->stream, d->d_enc_rows.p, B, d->nvar, d->tile(), io->out_first,
                 io->out_count, dst);
        LAUNCH_CHECK();
    } else {
        Timed t(d, LUTLDPC_K_FRONTEND);
        // one wave per output word that holds parity rows (at least one information-only word per wave where those are fewer)
        const int c_last = io->out_first + io->out_count - 1;
        const int n_par = c_last < K ? 0 : Wout - std::max(0, (K - io->out_first) / 32);
        const unsigned gx = (unsigned)((B + kEncFrames - 1) / kEncFrames), gy = (unsigned)std::max(1, (std::max(n_par, (Wout - n_par + 7) / 8) + 3) / 4);
        launch_k(encode_bits_kernel, dim3(gx, gy), dim3(256), (size_t)((K + 127) / 128) * kEncFrames * 16, d->stream, d->d_gen.p, K, R, d->gen_W32p, src, stride, B,
                 io->out_first, io->out_count, dst);
        LAUNCH_CHECK();
    }
    if (!dev && (rc = copy_to_host(d, out_words, dst, sizeof(uint32_t) * (size_t)B * (size_t)Wout))) return rc;
    if (!dev || io->sync) HIP_TRY(hipStreamSynchronize(d->stream));
    return LUTLDPC_OK;
}

int lutldpc_decoder_sample_labels(lutldpc_decoder *d, const lutldpc_channel_cells *cells, uint64_t seed, uint32_t stream, uint64_t frame0, int B,
                                  const uint8_t *codewords, uint8_t *cha, uint8_t *msg0) {
    if (!d || !cha || !msg0) return fail(LUTLDPC_ERR_ARG, "NULL argument");
    int rc = batch_entry(d, B, stream);
    if (rc) return rc;
    ChannelCells C;
    if ((rc = fill_cells(cells, d, C))) return rc;
    const uint8_t *sent_rows = nullptr;
    if ((rc = sent_rows_from_host(d, codewords, B, &sent_rows))) return rc;
    if ((rc = sample_tiles(d, C, seed, stream, frame0, B, sent_rows))) return rc;
    if ((rc = rows_to_host(d, d->d_cha_t.p, cha, B)) || (rc = rows_to_host(d, d->d_msg0_t.p, msg0, B))) return rc;
    HIP_TRY(hipStreamSynchronize(d->stream));
    return LUTLDPC_OK;
}

}  // extern "C"
