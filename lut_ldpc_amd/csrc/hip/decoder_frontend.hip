// decoder_frontend.hip -- the Monte-Carlo front end on the device: channel sampler, error counters and the C-ABI entries built on
// them (the sent bits come from decoder_encode.hip: sent_rows_of).  Home of every kernel of kernels_frontend.hpp.
#include "decoder_state.hpp"
#include "kernels_frontend.hpp"

#pragma GCC visibility push(hidden)

// (see preload_code_objects) this unit's code object
hipError_t preload_frontend_kernels() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&sample_labels_kernel<1>));
}

// instantiate a launch for the decoder's packing (PK) and for sent-bit rows or the all-zero codeword (SR)
#define PACK_SENT_DISPATCH(d, sent_rows, ...)                                        \
    do {                                                                             \
        if (sent_rows) { constexpr bool SR = true; PACK_DISPATCH(d, __VA_ARGS__); }  \
        else { constexpr bool SR = false; PACK_DISPATCH(d, __VA_ARGS__); }           \
    } while (0)

// a caller's cell table -> the image the sampler reads: the checks of the header's error contract, the thresholds and the packed
// labels of the cells (what lies past them stays zero: the image is also its key in the parameter arena), the bucket index
static int fill_table(const lutldpc_channel_cells *c, const lutldpc_decoder *d, NodeClassTable &T) {
    if (!c || !c->thr || !c->cha_label || !c->msg_label || !c->slicer_neg || !c->cha_label_mirror || !c->msg_label_mirror)
        return fail(LUTLDPC_ERR_ARG, "channel cells: NULL member");
    if (c->n_cells < 1 || c->n_cells > kMaxCells) return fail(LUTLDPC_ERR_ARG, "channel cells: n_cells outside [1,72]");
    std::memset(&T, 0, sizeof(T));
    T.n_thr = c->n_cells - 1;
    for (int j = 0; j < c->n_cells; j++) {
        if (j < T.n_thr) { T.thr[j] = c->thr[j]; if (j && c->thr[j] < c->thr[j - 1]) return fail(LUTLDPC_ERR_ARG, "channel cells: thresholds must ascend"); }
        if (c->cha_label[j] >= d->Nq_Cha || c->cha_label_mirror[j] >= d->Nq_Cha || c->msg_label[j] >= d->Nq_Msg[0] || c->msg_label_mirror[j] >= d->Nq_Msg[0])
            return fail(LUTLDPC_ERR_ARG, "channel cells: label outside its alphabet");
        T.attr[j] = (uint32_t)c->cha_label[j] | (c->slicer_neg[j] ? 1u << 7 : 0u) | ((uint32_t)c->msg_label[j] << 8) | ((uint32_t)c->cha_label_mirror[j] << 16) |
                    ((uint32_t)c->msg_label_mirror[j] << 24);
    }
    slice_index<kBucketBits>(T.thr, T.n_thr, T.first);
    return LUTLDPC_OK;
}

int front_end_of(const lutldpc_channel_cells *cells, lutldpc_decoder *d, FrontEnd &fe) {
    const lutldpc_decoder::NodeChannels &nc = d->node_channels;
    if (!cells && nc.n > 0) {
        fe = {reinterpret_cast<const NodeClassTable *>(nc.tables.p), nc.node_class.p, nc.n};
        return LUTLDPC_OK;
    }
    NodeClassTable T;
    if (int rc = fill_table(cells, d, T)) return rc;
    DEV_PARAM(dT, d, T);
    fe = {dT, nullptr, 1};
    return LUTLDPC_OK;
}

// sampler -> d_cha_t / d_msg0_t (tile layout); stats zeroed and slicer errors accumulated.  sent_rows: the sent bits of the
// batch (sent_rows_of), null = all-zero codeword
int sample_tiles(lutldpc_decoder *d, const FrontEnd &fe, uint64_t seed, uint32_t stream, uint64_t frame0, int B, const uint8_t *sent_rows) {
    int rc = ensure_batch(d, B);
    if (rc) return rc;
    const int Bpad = d->bpad(B), G = Bpad / d->tile(), N = d->nvar;
    // one slot without class bytes, or the handle's classes with a byte for every node
    if (!fe.tables || (fe.node_class ? fe.n_slots < 1 || fe.n_slots > kMaxNodeClasses || d->node_channels.node_class.n < (size_t)N : fe.n_slots != 1))
        return fail(LUTLDPC_ERR_STATE, "sampler: no node channels on the device");
    HIP_TRY(d->d_stats.alloc((size_t)Bpad * 4));
    HIP_TRY(hipMemsetAsync(d->d_stats.p, 0, sizeof(int32_t) * (size_t)Bpad * 4, d->stream));
    Timed t(d, LUTLDPC_K_FRONTEND);
    const int ppt = 8, npairs = (N + 1) / 2;
    dim3 grid((unsigned)((npairs + 4 * ppt - 1) / (4 * ppt)), (unsigned)G);
    PACK_SENT_DISPATCH(d, sent_rows, launch_k(sample_labels_kernel<PK, SR>, grid, dim3(256), (size_t)fe.n_slots * sizeof(NodeClassTable), d->stream, fe.tables, fe.node_class,
                                              fe.n_slots, (uint32_t)seed, (uint32_t)(seed >> 32), stream, frame0, B, N, sent_rows, d->d_cha_t.p, d->d_msg0_t.p, d->d_stats.p, ppt));
    LAUNCH_CHECK();
    return LUTLDPC_OK;
}

// lutldpc_decoder_sim_batch (codewords: host, frame-major, or null) and lutldpc_decoder_sim_batch_random (device_codewords:
// made by the encoder on the device from (seed, stream, frame))
int sim_batch_impl(lutldpc_decoder *d, const lutldpc_channel_cells *cells, uint64_t seed, uint32_t stream, uint64_t frame0, int B,
                   const uint8_t *codewords, bool device_codewords, int K_info, int32_t *frame_stats, uint8_t *cha_out, uint8_t *bits_out, lutldpc_event_request *req) {
    if (!d || !frame_stats) return fail(LUTLDPC_ERR_ARG, "NULL argument");
    int rc = batch_entry(d, B, stream);
    if (rc) return rc;
    if (K_info < 0 || K_info > d->nvar) return fail(LUTLDPC_ERR_ARG, "bad K_info");
    if (device_codewords && (rc = require_generator(d, "sim_batch_random: no generator set (lutldpc_decoder_set_generator)"))) return rc;
    FrontEnd fe;
    if ((rc = front_end_of(cells, d, fe))) return rc;
    const uint8_t *sent_rows = nullptr;
    if ((rc = sent_rows_of(d, codewords, device_codewords, seed, stream, frame0, B, &sent_rows))) return rc;
    if ((rc = sample_tiles(d, fe, seed, stream, frame0, B, sent_rows))) return rc;
    // the sampled labels, read back from the rows before the decode works on them: a decode that compacts leaves the channel rows
    // in slot order (launch_uncompaction brings back the decided bits and the iteration codes only)
    if (cha_out && (rc = rows_to_host(d, d->d_cha_t.p, cha_out, B))) return rc;
    if ((rc = decode_tiles(d, B))) return rc;
    {
        Timed t(d, LUTLDPC_K_FRONTEND);
        const int Bpad = d->bpad(B), G = Bpad / d->tile(), rpw = 64;
        const int rows = K_info > 0 ? K_info : 1;
        const dim3 grid((unsigned)((rows + 4 * rpw - 1) / (4 * rpw)), (unsigned)G);
        PACK_SENT_DISPATCH(d, sent_rows, launch_k(count_errors_kernel<PK, SR>, grid, dim3(256), 0, d->stream, d->d_hard.p, sent_rows, B, d->nvar, K_info, d->d_iters.p, d->d_stats.p, rpw));
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

int lutldpc_decoder_set_node_channels(lutldpc_decoder *d, const lutldpc_node_channels *nc) {
    if (!d) return fail(LUTLDPC_ERR_ARG, "NULL decoder");
    const int n = nc ? nc->n_classes : 0;
    if (n < 0 || n > LUTLDPC_MAX_NODE_CLASSES) return fail(LUTLDPC_ERR_ARG, "node channels: n_classes outside [0," + std::to_string(LUTLDPC_MAX_NODE_CLASSES) + "]");
    static_assert(LUTLDPC_MAX_NODE_CLASSES == kMaxNodeClasses, "the header's limit is the kernel's");
    std::vector<NodeClassTable> tables((size_t)n);
    std::vector<int> nodes((size_t)n, 0);
    if (n > 0) {
        if (!nc->tables || !nc->node_class) return fail(LUTLDPC_ERR_ARG, "node channels: NULL member");
        for (int c = 0; c < n; c++)
            if (int rc = fill_table(&nc->tables[c], d, tables[(size_t)c])) return rc;
        for (int v = 0; v < d->nvar; v++) {
            if (nc->node_class[v] >= n) return fail(LUTLDPC_ERR_ARG, "node channels: node_class[" + std::to_string(v) + "] outside [0, n_classes)");
            nodes[nc->node_class[v]]++;
        }
    }
    if (int rc = device_entry(d)) return rc;
    // Everything above refuses without touching the setting.  From here on only the HIP runtime can fail, and then no classes are
    // set.  The two buffers are allocated once, for the largest record (16 tables, nvar bytes), and written in place: a caller that
    // sets new tables for every SNR point or batch (the codec layer does) pays two small copies, no allocation.
    lutldpc_decoder::NodeChannels &cur = d->node_channels;
    HIP_TRY(hipStreamSynchronize(d->stream));      // (no sampler launch still reads the record)
    // describe() shows the classes and their node counts only; its checksums are not computed again where those stay
    const bool shown = n != cur.n || nodes != cur.nodes;
    cur.n = 0;
    if (n > 0) {
        HIP_TRY(cur.tables.alloc((size_t)kMaxNodeClasses * sizeof(NodeClassTable) / sizeof(uint64_t)));
        HIP_TRY(cur.node_class.alloc((size_t)d->nvar));
        HIP_TRY(hipMemcpy(cur.tables.p, tables.data(), (size_t)n * sizeof(NodeClassTable), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(cur.node_class.p, nc->node_class, (size_t)d->nvar, hipMemcpyHostToDevice));
        cur.n = n;
    } else {
        cur.tables.release();
        cur.node_class.release();
    }
    cur.nodes = nodes;
    if (shown) make_describe(d);
    return LUTLDPC_OK;
}

int lutldpc_decoder_sim_batch(lutldpc_decoder *d, const lutldpc_channel_cells *cells, uint64_t seed, uint32_t stream, uint64_t frame0, int B,
                              const uint8_t *codewords, int K_info, int32_t *frame_stats, uint8_t *cha_out, uint8_t *bits_out) {
    return sim_batch_impl(d, cells, seed, stream, frame0, B, codewords, false, K_info, frame_stats, cha_out, bits_out);
}

int lutldpc_decoder_sim_batch_random(lutldpc_decoder *d, const lutldpc_channel_cells *cells, uint64_t seed, uint32_t stream, uint64_t frame0, int B,
                                     int K_info, int32_t *frame_stats, uint8_t *cha_out, uint8_t *bits_out) {
    return sim_batch_impl(d, cells, seed, stream, frame0, B, nullptr, true, K_info, frame_stats, cha_out, bits_out);
}

int lutldpc_decoder_sample_labels(lutldpc_decoder *d, const lutldpc_channel_cells *cells, uint64_t seed, uint32_t stream, uint64_t frame0, int B,
                                  const uint8_t *codewords, uint8_t *cha, uint8_t *msg0) {
    if (!d || !cha || !msg0) return fail(LUTLDPC_ERR_ARG, "NULL argument");
    int rc = batch_entry(d, B, stream);
    if (rc) return rc;
    FrontEnd fe;
    if ((rc = front_end_of(cells, d, fe))) return rc;
    const uint8_t *sent_rows = nullptr;
    if ((rc = sent_rows_from_host(d, codewords, B, &sent_rows))) return rc;
    if ((rc = sample_tiles(d, fe, seed, stream, frame0, B, sent_rows))) return rc;
    if ((rc = rows_to_host(d, d->d_cha_t.p, cha, B)) || (rc = rows_to_host(d, d->d_msg0_t.p, msg0, B))) return rc;
    HIP_TRY(hipStreamSynchronize(d->stream));
    return LUTLDPC_OK;
}

}  // extern "C"
