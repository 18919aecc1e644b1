// decoder_events.hip -- failed frames captured on the device: the launches behind a lutldpc_event_request (weights of every frame,
// selection and compaction, the sorted lists of the kept frames) and the C-ABI entries built on them.  Home of every kernel of
// kernels_events.hpp.  Nothing here runs, and nothing is allocated, unless a capture entry is called.
#include "decoder_state.hpp"
#include "kernels_events.hpp"

#pragma GCC visibility push(hidden)

// (see preload_code_objects) this unit's code object
hipError_t preload_events_kernels() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&event_select_kernel));
}

int event_request_check(const lutldpc_event_request *req) {
    if (!req) return fail(LUTLDPC_ERR_ARG, "NULL event request");
    if (!req->events) return fail(LUTLDPC_ERR_ARG, "event request: events is NULL");
    if (req->max_frames < 0 || req->max_pos < 0 || req->max_chk < 0) return fail(LUTLDPC_ERR_ARG, "event request: negative size");
    if (req->select < LUTLDPC_EV_CODEWORD || req->select > LUTLDPC_EV_UNDETECTED) return fail(LUTLDPC_ERR_ARG, "event request: select outside [0,3]");
    if ((req->max_pos > 0 && !req->positions) || (req->max_chk > 0 && !req->checks))
        return fail(LUTLDPC_ERR_ARG, "event request: positions / checks may be NULL only when their maximum is 0");
    return LUTLDPC_OK;
}

// rows (checks) per run: about 512 runs per frame group where the code is long enough, never more than a byte can count
static int run_length(int n, int least) { return std::min(kEvMaxRun, std::max(least, (n + 511) / 512)); }

int capture_events(lutldpc_decoder *d, int B, int K_info, const uint8_t *sent_rows, const int32_t *stats, lutldpc_event_request *req) {
    lutldpc_decoder::Events &ev = d->ev;
    const int Bpad = d->bpad(B), G = Bpad / d->tile(), N = d->nvar, M = d->nchk;
    const int cap = std::min(req->max_frames, B);                      // slots that can be filled
    const int rpw = run_length(N, 16), n_runs_n = (N + rpw - 1) / rpw;
    const int cpw = run_length(M, 8), n_runs_c = (M + cpw - 1) / cpw;
    const bool want_pos = cap > 0 && req->max_pos > 0, want_chk = cap > 0 && req->max_chk > 0;
    const size_t n_pos = (size_t)cap * (size_t)req->max_pos, n_chk = (size_t)cap * (size_t)req->max_chk;
    HIP_TRY(ev.frame_w.alloc((size_t)Bpad * 4));
    HIP_TRY(ev.slot_of.alloc((size_t)Bpad));
    HIP_TRY(ev.counters.alloc(2));
    HIP_TRY(ev.records.alloc((size_t)std::max(cap, 1) * kEvRecord));
    HIP_TRY(hipMemsetAsync(ev.frame_w.p, 0, sizeof(int32_t) * (size_t)Bpad * 4, d->stream));
    if (want_pos) {
        HIP_TRY(ev.cnt_n.alloc((size_t)n_runs_n * Bpad)); HIP_TRY(ev.off_n.alloc((size_t)n_runs_n * cap)); HIP_TRY(ev.positions.alloc(n_pos));
        HIP_TRY(hipMemsetAsync(ev.positions.p, 0xFF, sizeof(int32_t) * n_pos, d->stream));
    }
    if (want_chk) {
        HIP_TRY(ev.cnt_c.alloc((size_t)n_runs_c * Bpad)); HIP_TRY(ev.off_c.alloc((size_t)n_runs_c * cap)); HIP_TRY(ev.checks.alloc(n_chk));
        HIP_TRY(hipMemsetAsync(ev.checks.p, 0xFF, sizeof(int32_t) * n_chk, d->stream));
    }
    if (req->node_errors) { HIP_TRY(ev.node_errors.alloc((size_t)N)); HIP_TRY(hipMemsetAsync(ev.node_errors.p, 0, sizeof(unsigned long long) * (size_t)N, d->stream)); }
    if (req->check_fails) { HIP_TRY(ev.check_fails.alloc((size_t)M)); HIP_TRY(hipMemsetAsync(ev.check_fails.p, 0, sizeof(unsigned long long) * (size_t)M, d->stream)); }
    const dim3 grid_n((unsigned)((n_runs_n + 3) / 4), (unsigned)G), grid_c((unsigned)((n_runs_c + 3) / 4), (unsigned)G);
    const uint32_t *cn_vnf = reinterpret_cast<const uint32_t *>(d->d_cn_vn.p);
    {
        Timed t(d, LUTLDPC_K_FRONTEND);
        PACK_DISPATCH(d, launch_k(event_weights_kernel<PK>, grid_n, dim3(256), 0, d->stream, d->d_hard.p, sent_rows, B, Bpad, N, K_info, rpw, ev.frame_w.p,
                                  req->node_errors ? ev.node_errors.p : nullptr, want_pos ? ev.cnt_n.p : nullptr));
        PACK_DISPATCH(d, launch_k(event_syndrome_kernel<PK>, grid_c, dim3(256), 0, d->stream, d->d_hard.p, d->d_cn_ptr.p, cn_vnf, B, Bpad, M, N, cpw, ev.frame_w.p,
                                  req->check_fails ? ev.check_fails.p : nullptr, want_chk ? ev.cnt_c.p : nullptr));
        launch_k(event_select_kernel, dim3(1), dim3(1024), 0, d->stream, ev.frame_w.p, d->d_iters.p, stats, B, Bpad, req->select, req->max_frames, req->max_pos,
                 req->max_chk, ev.records.p, ev.slot_of.p, ev.counters.p);
        if (want_pos || want_chk)
            launch_k(event_offsets_kernel, dim3((unsigned)((cap + 255) / 256), 2u), dim3(256), 0, d->stream, ev.records.p, ev.counters.p, cap, Bpad,
                     want_pos ? ev.cnt_n.p : nullptr, n_runs_n, ev.off_n.p, want_chk ? ev.cnt_c.p : nullptr, n_runs_c, ev.off_c.p);
        if (want_pos)
            PACK_DISPATCH(d, launch_k(event_fill_nodes_kernel<PK>, grid_n, dim3(256), 0, d->stream, d->d_hard.p, sent_rows, Bpad, N, rpw, ev.slot_of.p, ev.cnt_n.p,
                                      ev.off_n.p, cap, req->max_pos, ev.positions.p));
        if (want_chk)
            PACK_DISPATCH(d, launch_k(event_fill_checks_kernel<PK>, grid_c, dim3(256), 0, d->stream, d->d_hard.p, d->d_cn_ptr.p, cn_vnf, Bpad, M, N, cpw, ev.slot_of.p,
                                      ev.cnt_c.p, ev.off_c.p, cap, req->max_chk, ev.checks.p));
        LAUNCH_CHECK();
    }
    // what leaves the device: two counters, then the records and lists of the kept frames, then the profiles that were asked for
    int32_t counters[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(counters, ev.counters.p, sizeof(counters), hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    const size_t kept = (size_t)counters[1];
    if (kept > (size_t)cap) return fail(LUTLDPC_ERR_STATE, "capture: more frames stored than slots");
    std::vector<unsigned long long> pn, pc;
    if (kept) {
        HIP_TRY(hipMemcpyAsync(req->events, ev.records.p, sizeof(int32_t) * kept * kEvRecord, hipMemcpyDeviceToHost, d->stream));
        if (want_pos) HIP_TRY(hipMemcpyAsync(req->positions, ev.positions.p, sizeof(int32_t) * kept * (size_t)req->max_pos, hipMemcpyDeviceToHost, d->stream));
        if (want_chk) HIP_TRY(hipMemcpyAsync(req->checks, ev.checks.p, sizeof(int32_t) * kept * (size_t)req->max_chk, hipMemcpyDeviceToHost, d->stream));
    }
    if (req->node_errors) { pn.resize((size_t)N); HIP_TRY(hipMemcpyAsync(pn.data(), ev.node_errors.p, sizeof(unsigned long long) * (size_t)N, hipMemcpyDeviceToHost, d->stream)); }
    if (req->check_fails) { pc.resize((size_t)M); HIP_TRY(hipMemcpyAsync(pc.data(), ev.check_fails.p, sizeof(unsigned long long) * (size_t)M, hipMemcpyDeviceToHost, d->stream)); }
    HIP_TRY(hipStreamSynchronize(d->stream));
    for (size_t v = 0; v < pn.size(); v++) req->node_errors[v] += (int64_t)pn[v];
    for (size_t c = 0; c < pc.size(); c++) req->check_fails[c] += (int64_t)pc[c];
    req->n_selected = counters[0];
    req->n_stored = counters[1];
    return LUTLDPC_OK;
}

#pragma GCC visibility pop

extern "C" {

int lutldpc_decoder_events_batch(lutldpc_decoder *d, const uint8_t *cha, const uint8_t *msg0, const uint8_t *sent, int B, int K_info,
                                 uint8_t *out_bits, int32_t *out_iters, lutldpc_event_request *req) {
    int rc;
    if ((rc = event_request_check(req))) return rc;
    if (!d || !cha || !msg0) return fail(LUTLDPC_ERR_ARG, "NULL argument");
    if (K_info < 0 || K_info > d->nvar) return fail(LUTLDPC_ERR_ARG, "bad K_info");
    if ((rc = batch_entry(d, B))) return rc;
    const uint8_t *sent_rows = nullptr;
    if ((rc = tiles_from_host(d, cha, msg0, B)) || (rc = sent_rows_from_host(d, sent, B, &sent_rows))) return rc;
    if ((rc = decode_tiles(d, B))) return rc;
    if (out_bits && (rc = rows_to_host(d, d->d_hard.p, out_bits, B))) return rc;
    if (out_iters && (rc = iters_to_host(d, out_iters, B))) return rc;
    return capture_events(d, B, K_info, sent_rows, nullptr, req);
}

int lutldpc_decoder_sim_batch_events(lutldpc_decoder *d, const lutldpc_channel_cells *cells, uint64_t seed, uint32_t stream, uint64_t frame0,
                                     int B, const uint8_t *codewords, int device_codewords, int K_info, int32_t *frame_stats,
                                     lutldpc_event_request *req) {
    int rc;
    if ((rc = event_request_check(req))) return rc;
    if (!d || !frame_stats) return fail(LUTLDPC_ERR_ARG, "NULL argument");
    if (K_info < 0 || K_info > d->nvar) return fail(LUTLDPC_ERR_ARG, "bad K_info");
    return sim_batch_impl(d, cells, seed, stream, frame0, B, device_codewords ? nullptr : codewords, device_codewords != 0, K_info, frame_stats, nullptr, nullptr, req);
}

}  // extern "C"
