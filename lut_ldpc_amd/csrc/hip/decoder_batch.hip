// decoder_batch.hip -- the batch buffers of a decoder, the device arena of kernel parameter structures, the placement
// search for the row buffers of a large batch, and the entry layer: the guard, labels-in and results-out steps every batch
// entry of the C-ABI shares.
#include "decoder_state.hpp"

#pragma GCC visibility push(hidden)

// device copy of a parameter structure (see lutldpc_decoder::ParamArena); nullptr + last error on failure
constexpr size_t kParamChunk = 1u << 20;
const void *dev_param_bytes(lutldpc_decoder *d, const void *src, size_t n) {
    auto &A = d->params;
    std::string key((const char *)src, n);
    auto it = A.off_of.find(key);
    size_t off;
    if (it == A.off_of.end()) {
        const size_t need = (n + 63) / 64 * 64;
        if (A.chunks.empty() || A.used + need > A.cap) {
            if (A.chunks.size() >= 64) {          // 64 MB of distinct parameter blocks: a caller with ever-changing shapes -- start over
                (void)hipStreamSynchronize(d->stream);
                d->drop_graphs();
                A.clear();
            }
            DevBuf<uint8_t> c;
            if (c.alloc(std::max(kParamChunk, need)) != hipSuccess) { fail(LUTLDPC_ERR_HIP, "parameter arena: hipMalloc failed"); return nullptr; }
            A.chunk_base.push_back(A.cap);
            A.used = A.cap;
            A.cap += c.n;
            A.chunks.push_back(std::move(c));
        }
        off = A.used;
        A.used += need;
        it = A.off_of.emplace(std::move(key), off).first;
        const size_t ci = A.chunks.size() - 1;
        if (hipMemcpyAsync(A.chunks[ci].p + (off - A.chunk_base[ci]), it->first.data(), n, hipMemcpyHostToDevice, d->stream) != hipSuccess) {
            fail(LUTLDPC_ERR_HIP, "parameter arena: upload failed");
            return nullptr;
        }
    } else off = it->second;
    size_t ci = A.chunks.size() - 1;
    while (ci > 0 && A.chunk_base[ci] > off) ci--;
    return A.chunks[ci].p + (off - A.chunk_base[ci]);
}

// Placement search for the row buffers of a large batch.  Where they land in HBM decides 6 % of the decode rate (one process,
// fresh allocations of the same sizes: 241.8 ... 262.9 k codewords/s on DVB-S2, each level steady to 0.1 %;
// profiles/r03_level_probe_*.txt), and nothing visible from here predicts it -- so the first decode of a batch size tries up to
// opt.place_candidates allocations, times three iterations of the fused pipeline on each and keeps the fastest (it stops early
// once a candidate stands clear of the slowest seen).  LUTLDPC_PLACE=0 off, =n at most n candidates.  Candidate 0 is what ensure_batch
// has just allocated; every further candidate is a fresh set of the same sizes, ALL kept alive until the choice is made (a freed
// set would be handed out again).  The probe is the real thing on zeroed rows: frame states, then three iterations of the fused
// pipeline (six launches), timed with events on the decoder's stream; the second run counts.  Only for the skewed streaming path
// and batches whose rows exceed 1 GiB -- below that the launches are not bound by HBM.  Allocation failures end the search quietly.
static int place_rows(lutldpc_decoder *d, int Bpad) {
    const int G = Bpad / d->tile();
    const size_t total = d->d_msgs.bytes() + d->d_cha_t.bytes() + d->d_msg0_t.bytes() + d->d_hard.bytes();
    d->place_info = "null";
    if (d->opt.place_candidates < 2 || d->device < 0 || !d->opt.skew || !d->skew_ok || resident_active(d) || d->trace.level > 1 || total < ((size_t)1 << 30) || d->max_iters_created < 2) return LUTLDPC_OK;
    struct RowSet { DevBuf<uint8_t> msgs, cha, msg0, hard; float ms = 0.f; int id = 0; };
    std::vector<std::unique_ptr<RowSet>> parked;      // the candidates tried so far, except the one the decoder holds right now
    const size_t n_msgs = d->d_msgs.n, n_node = d->d_cha_t.n;
    auto swap_in = [&](RowSet &r) { std::swap(d->d_msgs, r.msgs); std::swap(d->d_cha_t, r.cha); std::swap(d->d_msg0_t, r.msg0); std::swap(d->d_hard, r.hard); };
    const int I0 = d->max_iters; const bool psc0 = d->psc, pisc0 = d->pisc; const int prof0 = d->profiling;
    d->max_iters = std::min(3, d->max_iters_created); d->psc = d->pisc = false; d->profiling = 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = LUTLDPC_OK;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { (void)hipGetLastError(); rc = -1; }
    std::vector<float> times;                          // probe time of every candidate, in the order tried
    size_t parked_bytes = 0, mem_free = 0, mem_total = 0;
    if (hipMemGetInfo(&mem_free, &mem_total) != hipSuccess) { (void)hipGetLastError(); mem_free = 0; }
    const size_t mem_budget = mem_free / 3;          // (a third: two lanes of a device may search at the same time)
    float cur_ms = 0.f; int cur_id = 0;                // the candidate the decoder holds
    for (int k = 0; k < d->opt.place_candidates && rc == LUTLDPC_OK; k++) {
        if (k > 0) {
            std::unique_ptr<RowSet> r(new RowSet());
            if (parked_bytes + 2 * total > mem_budget) break;      // keep the search within a third of what was free when it started
            if (r->msgs.alloc(n_msgs) != hipSuccess || r->cha.alloc(n_node) != hipSuccess || r->msg0.alloc(n_node) != hipSuccess || r->hard.alloc(n_node) != hipSuccess ||
                hipMemsetAsync(r->msgs.p, 0, r->msgs.bytes(), d->stream) != hipSuccess || hipMemsetAsync(r->cha.p, 0, r->cha.bytes(), d->stream) != hipSuccess ||
                hipMemsetAsync(r->msg0.p, 0, r->msg0.bytes(), d->stream) != hipSuccess || hipMemsetAsync(r->hard.p, 0, r->hard.bytes(), d->stream) != hipSuccess) {
                (void)hipGetLastError(); break;                     // out of memory: choose among what was tried
            }
            swap_in(*r);                               // the decoder works on candidate k, r holds candidate cur_id
            r->ms = cur_ms; r->id = cur_id;
            parked.push_back(std::move(r));
            parked_bytes += total;
            cur_id = k;
        }
        for (int rep = 0; rep < 2 && rc == LUTLDPC_OK; rep++) {
            if ((rc = launch_state(d, Bpad, Bpad, 0, 0))) break;
            if (hipEventRecord(e0, d->stream) != hipSuccess) { rc = -1; break; }
            if ((rc = iterate_skewed(d, Bpad, Bpad, G))) break;
            if (hipEventRecord(e1, d->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess) { rc = -1; break; }
            (void)hipEventElapsedTime(&cur_ms, e0, e1);
        }
        times.push_back(cur_ms);
        // the levels are discrete (on DVB-S2: 5.97 / 6.25 / 6.45-6.6 ms for the probe, the top one in one allocation out of eight):
        // stop as soon as one candidate stands 6.5 % clear of the slowest seen
        if (times.size() >= 4) {
            const float lo = *std::min_element(times.begin(), times.end()), hi = *std::max_element(times.begin(), times.end());
            if (lo <= 0.935f * hi) break;
        }
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    d->max_iters = I0; d->psc = psc0; d->pisc = pisc0; d->profiling = prof0;
    if (rc != LUTLDPC_OK) {        // a probe failed: keep what the decoder holds, report nothing (the decode that follows surfaces a real error)
        (void)hipGetLastError();
        return LUTLDPC_OK;
    }
    for (auto &c : parked)
        if (c->ms < cur_ms) { swap_in(*c); std::swap(c->ms, cur_ms); std::swap(c->id, cur_id); }      // the decoder ends up with the fastest set
    std::ostringstream o;
    o << "{\"candidates\":" << times.size() << ",\"chosen\":" << cur_id << ",\"probe_ms\":[";
    for (size_t k = 0; k < times.size(); k++) o << (k ? "," : "") << times[k];
    o << "]}";
    d->place_info = o.str();
    parked.clear();
    // the probes ran on zeroed rows and left their messages behind: defined content again (see ensure_batch)
    HIP_TRY(hipMemsetAsync(d->d_msgs.p, 0, d->d_msgs.bytes(), d->stream));
    HIP_TRY(hipMemsetAsync(d->d_hard.p, 0, d->d_hard.bytes(), d->stream));
    d->drop_graphs();
    make_describe(d);
    if (d->opt.debug_addr) fprintf(stderr, "lutldpc placement: %s -> msgs %p\n", d->place_info.c_str(), (void *)d->d_msgs.p);
    return LUTLDPC_OK;
}

int ensure_batch(lutldpc_decoder *d, int B) {
    int Bpad = d->bpad(B);
    if (Bpad <= d->Bcap) return LUTLDPC_OK;
    size_t G = (size_t)(Bpad / d->tile());
    d->drop_graphs();                                // the captured launches hold the old buffer addresses,
    d->drop_plans();                                 // the launch plans the strides of the flag buffers
    HIP_TRY(d->d_msgs.alloc(G * (size_t)d->E * kRowBytes));
    HIP_TRY(d->d_cha_t.alloc(G * (size_t)d->nvar * kRowBytes));
    HIP_TRY(d->d_msg0_t.alloc(G * (size_t)d->nvar * kRowBytes));
    HIP_TRY(d->d_hard.alloc(G * (size_t)d->nvar * kRowBytes));
    HIP_TRY(d->d_state.alloc((size_t)Bpad));
    HIP_TRY(d->d_vfail.alloc((size_t)Bpad * kVfailSlots * 2));  // two buffers (skewed pipeline: this / next exit test) of kVfailSlots copies, Bcap bytes apart
    HIP_TRY(d->d_iters.alloc((size_t)Bpad));
    HIP_TRY(d->d_frame_of.alloc((size_t)Bpad)); HIP_TRY(d->d_perm.alloc((size_t)Bpad)); HIP_TRY(d->d_tmp3.alloc((size_t)Bpad * 3));
    HIP_TRY(d->d_ctl.alloc(8)); HIP_TRY(d->d_slot_of.alloc((size_t)Bpad)); HIP_TRY(d->d_iters_tmp.alloc((size_t)Bpad));
    HIP_TRY(d->d_grp.alloc(G));
    // Every row exists with a defined content from the start: with the first check pass reading the initial-message rows
    // (first_from_nodes) the edge rows of PAD frames and of frames that passed the test on the channel decisions are never
    // written while their group still has active frames, and the variable passes compute on all lanes (results masked).
    HIP_TRY(hipMemsetAsync(d->d_msgs.p, 0, d->d_msgs.bytes(), d->stream));
    HIP_TRY(hipMemsetAsync(d->d_hard.p, 0, d->d_hard.bytes(), d->stream));
    HIP_TRY(hipMemsetAsync(d->d_cha_t.p, 0, d->d_cha_t.bytes(), d->stream));
    HIP_TRY(hipMemsetAsync(d->d_msg0_t.p, 0, d->d_msg0_t.bytes(), d->stream));
    d->Bcap = Bpad;
    if (d->opt.debug_addr)                   // (LUTLDPC_DEBUG_ADDR: where did the row buffers of this handle land?)
        fprintf(stderr, "lutldpc rows: msgs %p cha %p msg0 %p hard %p (%zu MB of messages)\n", (void *)d->d_msgs.p, (void *)d->d_cha_t.p, (void *)d->d_msg0_t.p, (void *)d->d_hard.p, d->d_msgs.bytes() >> 20);
    return place_rows(d, Bpad);
}

// Always on, O(1), before every decode: the batch buffers every kernel addresses rows in exist and hold Bpad frames.  (The one
// device fault this library has shown was a valid edge row off a NULL message base)
int check_batch_buffers(const lutldpc_decoder *d, int Bpad) {
    const size_t G = (size_t)(Bpad / d->tile());
    auto bad = [&](const char *what) { return fail(LUTLDPC_ERR_STATE, std::string("batch buffer check failed before the decode: ") + what); };
    if (Bpad <= 0 || Bpad > d->Bcap || Bpad % d->tile()) return bad("batch larger than the allocation");
    if (!d->d_msgs.p || d->d_msgs.n < G * (size_t)d->E * kRowBytes) return bad("message rows");
    if (!d->d_cha_t.p || d->d_cha_t.n < G * (size_t)d->nvar * kRowBytes) return bad("channel rows");
    if (!d->d_msg0_t.p || d->d_msg0_t.n < G * (size_t)d->nvar * kRowBytes) return bad("initial-message rows");
    if (!d->d_hard.p || d->d_hard.n < G * (size_t)d->nvar * kRowBytes) return bad("decided-bit rows");
    if (!d->d_state.p || d->d_state.n < (size_t)Bpad || !d->d_iters.p || d->d_iters.n < (size_t)Bpad) return bad("frame state");
    if (!d->d_vfail.p || d->d_vfail.n < (size_t)d->Bcap * kVfailSlots * 2) return bad("flag buffers");
    if (!d->d_fast_idx.p || !d->d_tables.p || !d->stream) return bad("static tables / stream");
    return LUTLDPC_OK;
}

// ----------------------------------------------------------------------------- entry layer (decoder_state.hpp)
int device_entry(lutldpc_decoder *d) {
    if (!d) return fail(LUTLDPC_ERR_ARG, "NULL decoder");
    if (d->device < 0) return fail(LUTLDPC_ERR_STATE, "decoder was created without a device (host-only handle)");
    HIP_TRY(hipSetDevice(d->device));
    return LUTLDPC_OK;
}
int batch_entry(lutldpc_decoder *d, int B, uint32_t stream) {
    if (!d) return fail(LUTLDPC_ERR_ARG, "NULL decoder");
    if (B <= 0) return fail(LUTLDPC_ERR_ARG, "B must be positive");
    if (int rc = lutldpc_check_stream(stream)) return rc;
    return device_entry(d);
}
#pragma GCC visibility pop
// The Philox counter word 3 is `stream` for the channel uniforms and `stream | 0x80000000` for the information bits
// (kernels_frontend.hpp, kernels_encode.hpp, host/ber_sim_driver.cpp): a stream with bit 31 set would draw its channel noise from
// the very blocks that make the data of stream & 0x7FFFFFFF, and send that stream's data.  (Exported for host_capi.cpp, whose
// wrappers make codewords on the host before they reach an entry here.)
extern "C" int lutldpc_check_stream(uint32_t stream) {
    if (stream > LUTLDPC_STREAM_MAX)
        return fail(LUTLDPC_ERR_ARG, "stream must be below 2^31: bit 31 separates the information-bit stream from the channel stream");
    return LUTLDPC_OK;
}
#pragma GCC visibility push(hidden)

int tiles_from_device(lutldpc_decoder *d, const uint8_t *d_cha, const uint8_t *d_msg0, int B) {
    int rc = ensure_batch(d, B);
    if (rc) return rc;
    const int G = d->bpad(B) / d->tile();
    Timed t(d, LUTLDPC_K_LAYOUT);
    if ((rc = launch_labels_in(d, d_cha, (size_t)d->nvar, false, d->d_cha_t.p, nullptr, nullptr, B, G, d->Nq_Cha - 1))) return rc;
    return launch_labels_in(d, d_msg0, (size_t)d->nvar, false, d->d_msg0_t.p, nullptr, nullptr, B, G, d->Nq_Msg[0] - 1);
}
int labels_from_host(lutldpc_decoder *d, const uint8_t *cha, const uint8_t *msg0, int B, size_t stride) {
    const size_t n = (size_t)B * stride;
    HIP_TRY(d->d_in_cha.alloc(n));
    HIP_TRY(hipMemcpyAsync(d->d_in_cha.p, cha, n, hipMemcpyHostToDevice, d->stream));
    if (!msg0) return LUTLDPC_OK;
    HIP_TRY(d->d_in_msg.alloc(n));
    HIP_TRY(hipMemcpyAsync(d->d_in_msg.p, msg0, n, hipMemcpyHostToDevice, d->stream));
    return LUTLDPC_OK;
}
int tiles_from_host(lutldpc_decoder *d, const uint8_t *cha, const uint8_t *msg0, int B) {
    if (int rc = labels_from_host(d, cha, msg0, B, (size_t)d->nvar)) return rc;
    return tiles_from_device(d, d->d_in_cha.p, d->d_in_msg.p, B);
}

int copy_to_host(lutldpc_decoder *d, void *host_dst, const void *src, size_t bytes) {
    HIP_TRY(hipMemcpyAsync(host_dst, src, bytes, hipMemcpyDeviceToHost, d->stream));
    return LUTLDPC_OK;
}
int rows_to_host(lutldpc_decoder *d, const uint8_t *rows, uint8_t *host_dst, int B, int n_rows) {
    const size_t n = (size_t)B * (size_t)(n_rows > 0 ? n_rows : d->nvar);
    HIP_TRY(d->d_out_bits.alloc(n));
    {
        Timed t(d, LUTLDPC_K_LAYOUT);
        if (int rc = launch_transpose_out(d, rows, d->d_out_bits.p, B, d->bpad(B) / d->tile(), n_rows)) return rc;
    }
    return copy_to_host(d, host_dst, d->d_out_bits.p, n);
}
int iters_to_host(lutldpc_decoder *d, int32_t *dst, int B) { return copy_to_host(d, dst, d->d_iters.p, sizeof(int32_t) * (size_t)B); }

int check_out_window(const lutldpc_decoder *d, int first, int count) {
    if (first < 0 || count < 1 || (int64_t)first + count > d->nvar) return fail(LUTLDPC_ERR_ARG, "output window outside [0, nvar)");
    return LUTLDPC_OK;
}
int bits_to_caller(lutldpc_decoder *d, uint32_t *words, bool on_device, int B, int first, int count) {
    const size_t n = (size_t)B * (size_t)((count + 31) / 32);
    uint32_t *dst = words;
    if (!on_device) { HIP_TRY(d->d_out_words.alloc(n)); dst = d->d_out_words.p; }
    {
        Timed t(d, LUTLDPC_K_LAYOUT);
        if (int rc = launch_bits_out(d, dst, B, d->bpad(B) / d->tile(), first, count)) return rc;
    }
    return on_device ? LUTLDPC_OK : copy_to_host(d, words, dst, sizeof(uint32_t) * n);
}

#pragma GCC visibility pop
