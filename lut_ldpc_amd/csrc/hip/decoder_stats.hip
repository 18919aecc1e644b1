// decoder_stats.hip -- message-label histograms per dump, counted on the device: the edge grouping, the counted decode (a
// streaming decode with the exit tests off whose dumps go to message_histogram_kernel instead of the host) and the C-ABI
// entries built on it.  Home of every kernel of kernels_stats.hpp.
#include "decoder_state.hpp"
#include "kernels_stats.hpp"

#pragma GCC visibility push(hidden)

// (see preload_code_objects) this unit's code object; a 128-label alphabet takes 64 KB of dynamic LDS per workgroup
hipError_t preload_stats_kernels() {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&message_histogram_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, kHistMaxLabels * 512);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(&message_histogram_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, kHistMaxLabels * 512);
}

static int max_msg_alphabet(const lutldpc_decoder *d) { return *std::max_element(d->Nq_Msg.begin(), d->Nq_Msg.end()); }

// edges sorted by group (stable: ascending edge id inside a group); hist_run[0 .. n_groups] = where every group's run begins
static void build_edge_groups(lutldpc_decoder *d, const int32_t *edge_group, int n_groups) {
    const int E = d->E;
    std::vector<int32_t> start((size_t)n_groups + 1, 0);
    for (int e = 0; e < E; e++) start[(size_t)(edge_group ? edge_group[e] : 0) + 1]++;
    for (int g = 0; g < n_groups; g++) start[(size_t)g + 1] += start[(size_t)g];
    d->hist_edges.assign((size_t)E, 0);
    std::vector<int32_t> fill(start.begin(), start.end() - 1);
    for (int e = 0; e < E; e++) d->hist_edges[(size_t)fill[(size_t)(edge_group ? edge_group[e] : 0)]++] = e;
    d->hist_run = std::move(start);
    d->hist_groups = n_groups;
    d->hist_chunk_edges = 0;                            // chunk table and uploads: at the next counted decode
}

// Every group's run cut into chunks of `per` edges for a batch of G frame groups: about 4096 workgroups per launch where the
// code is large enough (each ends with up to 2 * Q atomics on the same few lines), between kHistChunkMin and kHistChunkEdges
// edges each.  Rebuilt (and uploaded) only when the size changes.
static int upload_edge_groups(lutldpc_decoder *d, int G) {
    if (d->hist_edges.empty()) build_edge_groups(d, nullptr, 1);
    int per = kHistChunkMin;
    while (per < kHistChunkEdges && (long long)d->E * G / per > 4096) per *= 2;
    if (per == d->hist_chunk_edges) return LUTLDPC_OK;
    d->hist_chunks.clear();
    for (int g = 0; g < d->hist_groups; g++)
        for (int p = d->hist_run[(size_t)g]; p < d->hist_run[(size_t)g + 1]; p += per) {
            d->hist_chunks.push_back(p);
            d->hist_chunks.push_back(std::min(per, d->hist_run[(size_t)g + 1] - p));
            d->hist_chunks.push_back(g);
        }
    HIP_TRY(hipStreamSynchronize(d->stream));           // (a counted decode in flight may still read the previous tables)
    HIP_TRY(d->d_hist_edges.upload(d->hist_edges));
    HIP_TRY(d->d_hist_chunks.upload(d->hist_chunks));
    d->hist_chunk_edges = per;
    return LUTLDPC_OK;
}

// one dump of a counted decode (decode_tiles_launch -> trace_dump): every message row of the batch, read once
int hist_dump(lutldpc_decoder *d) {
    lutldpc_decoder::Trace &T = d->trace;
    if (T.n >= T.n_dumps) return fail(LUTLDPC_ERR_STATE, "histogram: more dumps than the histogram holds");
    const int G = d->bpad(T.B) / d->tile(), Q = max_msg_alphabet(d), W = hist_waves(Q);
    const unsigned n_chunks = (unsigned)(d->hist_chunks.size() / 3);
    unsigned long long *slab = T.hist + (size_t)T.n * (size_t)d->hist_groups * 2 * (size_t)T.n_labels;
    Timed t(d, LUTLDPC_K_HISTOGRAM);
    PACK_DISPATCH(d, launch_k(message_histogram_kernel<PK>, dim3(n_chunks, (unsigned)G), dim3((unsigned)W * kWave), (size_t)W * Q * 512, d->stream, d->d_msgs.p,
                              d->d_hist_edges.p, d->d_hist_chunks.p, d->d_edge_vn.p, T.sent, T.last_dump, slab, d->E, d->nvar, T.n, Q, T.n_labels));
    LAUNCH_CHECK();
    T.n++;
    return LUTLDPC_OK;
}

// what both entries check before anything touches the device; *n_dumps_out = dumps of `level`
static int hist_check_args(lutldpc_decoder *d, int B, int level, int mode, int n_labels, const int64_t *hist, int64_t hist_cap, int *n_dumps_out,
                           uint32_t stream = 0) {
    if (!d || !hist) return fail(LUTLDPC_ERR_ARG, "NULL argument");
    if (level < 2 || level > 3) return fail(LUTLDPC_ERR_ARG, "histogram level must be 2 or 3");
    if (mode < 0 || mode > 1) return fail(LUTLDPC_ERR_ARG, "histogram mode must be 0 (all) or 1 (active)");
    if (n_labels < max_msg_alphabet(d)) return fail(LUTLDPC_ERR_ARG, "n_labels below the largest message alphabet (" + std::to_string(max_msg_alphabet(d)) + ")");
    const int nd = 1 + d->max_iters * (level - 1);
    const int64_t need = (int64_t)nd * d->hist_groups * 2 * n_labels;
    if (hist_cap < need) return fail(LUTLDPC_ERR_ARG, "hist too small: " + std::to_string(need) + " int64 needed");
    *n_dumps_out = nd;
    return batch_entry(d, B, stream);
}

// Does a normal decode of G frame groups move channel rows?  Only the compaction of the skewed pipeline does (launch_compaction
// permutes d_msgs and d_cha_t; launch_uncompaction brings back the decided bits and the iteration codes, not the labels).  No
// other kernel writes d_cha_t / d_msg0_t: the passes, the resident decoder and the exit tests only read them.
static bool decode_moves_labels(const lutldpc_decoder *d, int G) {
    return !resident_active(d) && d->opt.skew && d->skew_ok && d->psc && compaction_on(d, G);
}

// restores the exit conditions and the trace sink of a handle on every way out of the counted pass
struct CountedScope {
    lutldpc_decoder *d; int psc, pisc;
    explicit CountedScope(lutldpc_decoder *d_) : d(d_), psc(d_->psc), pisc(d_->pisc) { d->psc = 0; d->pisc = 0; }
    ~CountedScope() { d->psc = psc; d->pisc = pisc; d->trace = lutldpc_decoder::Trace(); }
};

// The labels of B frames are in tile layout (d_cha_t / d_msg0_t): decode them normally where the return values or the
// decided bits are wanted, then count the dumps of a second pass with the exit tests off.  refill(): writes the labels again.
template <class Refill>
static int histogram_tiles(lutldpc_decoder *d, int B, int level, int mode, int n_labels, const uint8_t *sent_rows, Refill &&refill,
                           uint8_t *out_bits, int32_t *out_iters, int64_t *hist, int n_dumps) {
    int rc;
    const int Bpad = d->bpad(B), G = Bpad / d->tile();
    if ((rc = upload_edge_groups(d, G))) return rc;
    const size_t n_hist = (size_t)n_dumps * (size_t)d->hist_groups * 2 * (size_t)n_labels;
    HIP_TRY(d->d_hist.alloc(n_hist));
    HIP_TRY(d->d_last_dump.alloc((size_t)Bpad));
    HIP_TRY(hipMemsetAsync(d->d_hist.p, 0, n_hist * sizeof(unsigned long long), d->stream));
    if (mode == 1 || out_bits || out_iters) {
        if ((rc = decode_tiles(d, B))) return rc;
        if (out_bits && (rc = rows_to_host(d, d->d_hard.p, out_bits, B))) return rc;
        if (out_iters && (rc = iters_to_host(d, out_iters, B))) return rc;
    }
    {
        Timed t(d, LUTLDPC_K_LAYOUT);
        launch_k(last_dump_kernel, dim3((unsigned)((Bpad + 255) / 256)), dim3(256), 0, d->stream, d->d_iters.p, B, Bpad, d->max_iters, level - 1, mode, n_dumps, d->d_last_dump.p);
        LAUNCH_CHECK();
    }
    if (mode == 1 || out_bits || out_iters)
        if (decode_moves_labels(d, G) && (rc = refill())) return rc;
    {
        CountedScope scope(d);
        lutldpc_decoder::Trace &T = d->trace;
        T.level = level; T.B = B; T.n = 0; T.hist = d->d_hist.p; T.sent = sent_rows; T.last_dump = d->d_last_dump.p; T.n_labels = n_labels; T.n_dumps = n_dumps;
        rc = decode_tiles(d, B);
        if (rc == LUTLDPC_OK && T.n != n_dumps) rc = fail(LUTLDPC_ERR_STATE, "histogram: the counted decode made " + std::to_string(T.n) + " dumps, expected " + std::to_string(n_dumps));
    }
    if (rc) return rc;
    std::vector<unsigned long long> h(n_hist);
    if ((rc = copy_to_host(d, h.data(), d->d_hist.p, n_hist * sizeof(unsigned long long)))) return rc;
    HIP_TRY(hipStreamSynchronize(d->stream));
    for (size_t i = 0; i < n_hist; i++) hist[i] += (int64_t)h[i];
    return LUTLDPC_OK;
}

#pragma GCC visibility pop

extern "C" {

int lutldpc_decoder_set_edge_groups(lutldpc_decoder *d, const int32_t *edge_group, int n_groups) {
    if (!d) return fail(LUTLDPC_ERR_ARG, "NULL decoder");
    if (n_groups < 1 || n_groups > 256) return fail(LUTLDPC_ERR_ARG, "n_groups outside [1,256]");
    if (edge_group)
        for (int e = 0; e < d->E; e++)
            if (edge_group[e] < 0 || edge_group[e] >= n_groups) return fail(LUTLDPC_ERR_ARG, "edge_group[" + std::to_string(e) + "] outside [0, n_groups)");
    build_edge_groups(d, edge_group, n_groups);
    return LUTLDPC_OK;
}

int lutldpc_decoder_histogram_shape(lutldpc_decoder *d, int level, int32_t *out4) {
    if (!d || !out4) return fail(LUTLDPC_ERR_ARG, "NULL argument");
    if (level < 2 || level > 3) return fail(LUTLDPC_ERR_ARG, "histogram level must be 2 or 3");
    out4[0] = 1 + d->max_iters * (level - 1); out4[1] = d->hist_groups; out4[2] = max_msg_alphabet(d); out4[3] = d->E;
    return LUTLDPC_OK;
}

int lutldpc_decoder_histogram_batch(lutldpc_decoder *d, const uint8_t *cha, const uint8_t *msg0, const uint8_t *sent, int B, int level, int mode,
                                    int n_labels, uint8_t *out_bits, int32_t *out_iters, int64_t *hist, int64_t hist_cap, int32_t *n_dumps) {
    int nd = 0, rc;
    if ((rc = hist_check_args(d, B, level, mode, n_labels, hist, hist_cap, &nd))) return rc;
    if (!cha || !msg0) return fail(LUTLDPC_ERR_ARG, "NULL argument");
    if ((rc = tiles_from_host(d, cha, msg0, B))) return rc;
    const uint8_t *sent_rows = nullptr;
    if ((rc = sent_rows_from_host(d, sent, B, &sent_rows))) return rc;
    auto refill = [&]() -> int { return tiles_from_device(d, d->d_in_cha.p, d->d_in_msg.p, B); };       // (the uploaded labels are still there)
    if ((rc = histogram_tiles(d, B, level, mode, n_labels, sent_rows, refill, out_bits, out_iters, hist, nd))) return rc;
    if (n_dumps) *n_dumps = nd;
    return LUTLDPC_OK;
}

int lutldpc_decoder_sim_batch_histogram(lutldpc_decoder *d, const lutldpc_channel_cells *cells, uint64_t seed, uint32_t stream, uint64_t frame0,
                                        int B, const uint8_t *codewords, int device_codewords, int level, int mode, int n_labels,
                                        int64_t *hist, int64_t hist_cap, int32_t *n_dumps) {
    int nd = 0, rc;
    if ((rc = hist_check_args(d, B, level, mode, n_labels, hist, hist_cap, &nd, stream))) return rc;
    if (device_codewords && (rc = require_generator(d, "sim_batch_histogram: no generator set (lutldpc_decoder_set_generator)"))) return rc;
    FrontEnd fe;
    if ((rc = front_end_of(cells, d, fe))) return rc;
    const uint8_t *sent_rows = nullptr;
    if ((rc = sent_rows_of(d, codewords, device_codewords != 0, seed, stream, frame0, B, &sent_rows))) return rc;
    auto fill = [&]() -> int { return sample_tiles(d, fe, seed, stream, frame0, B, sent_rows); };   // (a pure function of seed, stream, frame)
    if ((rc = fill())) return rc;
    if ((rc = histogram_tiles(d, B, level, mode, n_labels, sent_rows, fill, nullptr, nullptr, hist, nd))) return rc;
    if (n_dumps) *n_dumps = nd;
    return LUTLDPC_OK;
}

}  // extern "C"
