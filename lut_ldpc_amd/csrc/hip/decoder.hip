// decoder.hip -- C-ABI of the MI355X LUT-LDPC decode path (include/lut_ldpc_hip.h): creation with the table of run-time knobs,
// destruction, exit conditions, the decode entries, profiling, describe() and the self-test hooks.  decoder_state.hpp maps the units.
#include "decoder_state.hpp"

#include <climits>
#include <cstdlib>

#pragma GCC visibility push(hidden)

static thread_local std::string g_err;
int fail(int code, const std::string &msg) { g_err = msg; return code; }

// ----------------------------------------------------------------------------- profiling
hipEvent_t ev_get(lutldpc_decoder *d) {
    if (!d->ev_pool.empty()) { hipEvent_t e = d->ev_pool.back(); d->ev_pool.pop_back(); return e; }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}
void prof_fold(lutldpc_decoder *d) {
    if (d->ev_live.empty()) return;
    (void)hipStreamSynchronize(d->stream);
    for (auto &e : d->ev_live) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) { d->prof_ms[e.kind] += ms; d->prof_n[e.kind]++; }
        d->ev_pool.push_back(e.a); d->ev_pool.push_back(e.b);
    }
    d->ev_live.clear();
}

// CRC-32 (IEEE, reflected), chainable: crc32(crc32(0, a), b) = crc32 of a followed by b
static uint32_t crc32(uint32_t crc, const void *p, size_t n) {
    crc = ~crc;
    for (size_t i = 0; i < n; i++) {
        crc ^= static_cast<const uint8_t *>(p)[i];
        for (int k = 0; k < 8; k++) crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
    }
    return ~crc;
}

void make_describe(lutldpc_decoder *d) {
    std::ostringstream o;
    o << "{\"build\":\"" << __DATE__ << " " << __TIME__ << "\",\"kernel_sources\":\"" <<
#include "kernel_src_hash.inc"
      << "\",\"tile_frames\":" << d->tile() << ",\"message_bytes\":" << (d->pack == 2 ? "0.5" : "1") << ",\"pack\":" << d->pack << ",\"vector_bytes_per_lane\":4"
      << ",\"nodes_per_block\":" << d->opt.nodes_per_block << ",\"vn_edges_per_wave\":" << d->opt.vn_edges_per_wave << ",\"cn_edges_per_wave\":" << d->cn_epw() << ",\"use_fast\":" << d->opt.use_fast
      // knobs as given (0: unset, derived per degree class -- the classes below report what is in force)
      << ",\"nodes_per_wave\":" << d->opt.nodes_per_wave << ",\"nodes_per_wave_cn\":" << d->opt.nodes_per_wave_cn << ",\"tail_front\":" << d->opt.tail_front
      << ",\"fused_prio\":" << d->opt.fused_prio << ",\"chk_full_labels\":" << d->opt.chk_full_labels
      << ",\"vn_classes\":[";
    // the kernels of a class over the iterations (pass_kernel decides per iteration: a schedule that mixes power-of-two and other
    // message alphabets runs two of them), distinct names joined with '+' in the order fast, generated, interpreter
    const int I = d->max_iters_created;
    auto kernels_of = [&](int kind, size_t i, const char *const (&name)[3]) {
        bool used[3] = {false, false, false};
        if (kind == TT_VAR)         // variable pass ii writes the alphabet of iteration ii + 1 (a code of one iteration has none: set 0 decides)
            for (int ii = 0; ii < std::max(I - 1, 1); ii++) used[pass_kernel(d, TT_VAR, d->iter_set[(size_t)ii], (int)i, d->Nq_Msg[(size_t)std::min(ii + 1, I - 1)] / 2)] = true;
        else
            for (int ii = 0; ii < I; ii++) used[pass_kernel(d, TT_CHK, d->iter_set[(size_t)ii], (int)i, d->Nq_Msg[(size_t)ii] / 2)] = true;
        std::string s;
        for (int k = 0; k < 3; k++) if (used[k]) s += (s.empty() ? "" : "+") + std::string(name[k]);
        return s;
    };
    // the compile-time variable kernel of the class reads the root table as packed 64-bit rows (ClassParams::root_rows) in some iteration
    auto root_rows_of = [&](size_t i) {
        for (int ii = 0; ii < std::max(I - 1, 1); ii++)
            if (vn_root_rows(TT_VAR, d->pack, d->vclass[i].deg) && pass_kernel(d, TT_VAR, d->iter_set[(size_t)ii], (int)i, d->Nq_Msg[(size_t)std::min(ii + 1, I - 1)] / 2) == KERNEL_FAST) return true;
        return false;
    };
    for (size_t i = 0; i < d->vclass.size(); i++)
        o << (i ? "," : "") << "{\"deg\":" << d->vclass[i].deg << ",\"nodes\":" << d->vclass[i].nodes.size() << ",\"nodes_per_wave\":" << d->npw_vn(d->vclass[i].deg) << ",\"kernel\":\""
          << kernels_of(TT_VAR, i, {"vn_balanced_fast_kernel", "lutldpc_jit_pass", "tree_pass_kernel<VAR>"}) << "\",\"root_rows\":" << (root_rows_of(i) ? 1 : 0) << "}";
    o << "],\"cn_classes\":[";
    for (size_t i = 0; i < d->cclass.size(); i++) {
        // degree-2 nodes updated inside the check pass of this class: the forward links of its chain table (build_fast_index)
        int chained = 0;
        if (d->opt.use_chain && d->cclass[i].chain_off >= 0)
            for (size_t j = 0; j < d->cclass[i].nodes.size(); j++) chained += d->fast_idx[(size_t)d->cclass[i].chain_off + 2 * j + 1] != 0;
        o << (i ? "," : "") << "{\"deg\":" << d->cclass[i].deg << ",\"nodes\":" << d->cclass[i].nodes.size() << ",\"nodes_per_wave\":" << d->npw_cn_class(i)
          << ",\"chain_nodes\":" << chained << ",\"kernel\":\""
          << kernels_of(TT_CHK, i, {"cn_minsum_fast_kernel", "lutldpc_jit_pass", d->min_lut ? "cn_minsum_generic_kernel" : "tree_pass_kernel<CHK>"}) << "\"}";
    }
    o << "],\"resident\":" << (resident_active(d) ? 1 : 0) << ",\"skewed_pipeline\":" << ((d->opt.skew && d->skew_ok) ? 1 : 0) << ",\"fused_bucket\":" << d->fused_bucket_id << ",\"compaction\":" << (d->opt.use_compact < 0 ? 2 : d->opt.use_compact) << ",\"compaction_min_groups\":" << compaction_min_groups(d) << ",\"chain_nodes\":" << (d->opt.use_chain ? d->n_chain_nodes : 0) << ",\"placement\":" << d->place_info;
    if (const lutldpc_decoder::NodeChannels &nc = d->node_channels; nc.n > 0) {
        o << ",\"node_channels\":{\"classes\":" << nc.n << ",\"nodes\":[";
        for (int c = 0; c < nc.n; c++) o << (c ? "," : "") << nc.nodes[(size_t)c];
        o << "]}";
    }
    if (const lutldpc_decoder::Generator &gen = d->gen; gen.form != lutldpc_decoder::Generator::NONE) {
        o << ",\"generator\":{\"K\":" << gen.K << ",\"R\":" << gen.R;
        if (gen.form == lutldpc_decoder::Generator::SPARSE) o << ",\"form\":\"sparse\",\"terms\":" << gen.sparse.terms << ",\"block\":" << gen.sparse.block << ",\"depth\":" << gen.sparse.depth;
        o << "}";
    }
    {   // the static blobs, comparable between builds without a device.  (An Op has two bytes of padding before `mult`.)
        uint32_t ops = 0;
        for (const Op &op : d->all_ops) ops = crc32(crc32(ops, &op, offsetof(Op, child) + sizeof(op.child)), &op.mult, sizeof(Op) - offsetof(Op, mult));
        char b[160];
        snprintf(b, sizeof(b), ",\"static\":{\"ops\":%zu,\"ops_crc\":\"%08x\",\"tables_bytes\":%zu,\"tables_crc\":\"%08x\",\"index_words\":%zu,\"index_crc\":\"%08x\"}", d->all_ops.size(), ops,
                 d->all_tables.size(), crc32(0, d->all_tables.data(), d->all_tables.size()), d->fast_idx.size(), crc32(0, d->fast_idx.data(), 4 * d->fast_idx.size()));
        o << b;
    }
    o << "}";
    d->describe = o.str();
}

// ----------------------------------------------------------------------------- run-time knobs
// Every environment variable the decoder reads, each once, at creation (before compile_all).  An unset variable leaves the
// default of lutldpc_decoder::Options; a value outside [lo, hi] is ignored, not clamped.  DESIGN.md section 3 is written from
// this table.
using Options = lutldpc_decoder::Options;
enum KnobType { FLAG, INT, REAL, REAL_BELOW };      // FLAG: 0 / non-zero -> 0 / 1; INT, REAL: lo <= v <= hi; REAL_BELOW: lo <= v < hi
struct Knob { const char *name; KnobType type; int Options::*i; double Options::*r; double lo, hi; const char *meaning; };
#define KNOB_F(name, field, meaning) {name, FLAG, &Options::field, nullptr, 0, 1, meaning}
#define KNOB_I(name, field, lo, hi, meaning) {name, INT, &Options::field, nullptr, lo, hi, meaning}
#define KNOB_R(name, type, field, lo, hi, meaning) {name, type, nullptr, &Options::field, lo, hi, meaning}
static const Knob kKnobs[] = {
    // ---- kernel choice
    KNOB_F("LUTLDPC_USE_FAST", use_fast, "1: compile-time specialised kernels (and with them the fused pipeline, the generated kernels, the resident decoder); 0: interpreter kernels only"),
    KNOB_F("LUTLDPC_JIT", use_jit, "1: run-time generated kernels for shapes the compile-time path does not cover (jit.hpp)"),
    KNOB_I("LUTLDPC_PACK", pack, 1, 1, "1: byte rows even where every alphabet has <= 16 labels (unset: nibble rows there; on them the compile-time variable kernels of degree >= 3 read the root table as packed 64-bit rows, describe(): root_rows)"),
    KNOB_F("LUTLDPC_CHK_FULL", chk_full_labels, "1: generated check kernels on full-label tables; 0: on (sign, magnitude) tables as the reference walks them"),
    KNOB_F("LUTLDPC_CHAIN", use_chain, "1: degree-2 nodes between neighbouring checks of a wave are updated inside the check pass (build_fast_index)"),
    KNOB_F("LUTLDPC_LATE_HARD", late_hard, "1: decided bits of early-terminated frames recovered once, at the end, from their frozen messages; 0: stored by every variable pass"),
    KNOB_F("LUTLDPC_FIRST_FROM_NODES", first_from_nodes, "1: the first check pass reads the initial-message rows; 0: init_edges_kernel copies them to the edge rows first"),
    // ---- work per wave / block.  Measured on MI355X (DVB-S2, 4096 frames, repeated runs): short waves win -- 2 degree-8 nodes /
    // 6 degree-7 checks per wave (longer check runs also keep more chain nodes inside a wave).
    KNOB_I("LUTLDPC_NODES_PER_BLOCK", nodes_per_block, 1, 4096, "interpreter kernels: nodes per 64-thread block"),
    KNOB_I("LUTLDPC_NODES_PER_WAVE", nodes_per_wave, 1, 4096, "specialised kernels: fixed nodes per wave, variable AND check side (unset: edges per wave / degree)"),
    KNOB_I("LUTLDPC_NODES_PER_WAVE_CN", nodes_per_wave_cn, 1, 4096, "... check side only (overrides LUTLDPC_NODES_PER_WAVE there)"),
    KNOB_I("LUTLDPC_VN_EDGES_PER_WAVE", vn_edges_per_wave, 1, 65536, "variable side: edges per wave"),
    KNOB_I("LUTLDPC_CN_EDGES_PER_WAVE", cn_edges_per_wave, 1, 65536, "check side: edges per wave (unset: 42, chain-rich classes widened by build_fast_index; given: no widening)"),
    // ---- skewed pipeline
    KNOB_F("LUTLDPC_SKEW", skew, "1: two-half skewed pipeline through pass_fused_kernel where every class has a case in it"),
    KNOB_I("LUTLDPC_FUSED_BUCKET_MIN", fused_bucket_min, 0, kFusedBuckets - 1, "run a code of small degrees through a wider bucket's fused kernel (can only widen; what a bucket costs)"),
    KNOB_F("LUTLDPC_PRIO", fused_prio, "1: the look-up-heavy (variable) waves of the fused kernel raise their issue priority (no gain measured)"),
    KNOB_R("LUTLDPC_TAIL_FRONT", REAL_BELOW, tail_front, 0, 0.9, "fused launches: share of the item list that the slowest role stays clear of at the end"),
    KNOB_I("LUTLDPC_PLACE", place_candidates, 0, 32, "placement search of the row buffers: at most n candidate allocations, 0 / 1: off (place_rows)"),
    KNOB_F("LUTLDPC_GRAPH", use_graph, "1: repeated decodes replayed as one hipGraph launch"),
    // ---- compaction of the surviving frames (kernels_compact.hpp)
    KNOB_F("LUTLDPC_COMPACT", use_compact, "1 / 0: on / off (unset: automatic, long iterations only -- compaction_on)"),
    KNOB_I("LUTLDPC_COMPACT_FIRST", compact_first, 1, INT_MAX, "first iteration with a check point"),
    KNOB_I("LUTLDPC_COMPACT_EVERY", compact_every, 1, INT_MAX, "iterations between check points (unset: 2)"),
    KNOB_R("LUTLDPC_COMPACT_MARGIN", REAL_BELOW, compact_margin, 0, 100, "permute when the remaining iterations pay for it by this factor (0: whenever a group falls idle)"),
    KNOB_R("LUTLDPC_COMPACT_MIN_SHARE", REAL, compact_min_share, 0, 1, "... and at least this share of the live groups falls idle at once"),
    // ---- LDS-resident decoder (jit_resident.hpp)
    KNOB_I("LUTLDPC_RESIDENT", use_resident, INT_MIN, INT_MAX, "0: off (streaming kernels); 1: where the code fits and it pays; >= 2: wherever it fits"),
    KNOB_I("LUTLDPC_RESIDENT_S", resident_force_S, 1, 64, "sets (64 frames each) per workgroup (unset: resident_pick)"),
    KNOB_I("LUTLDPC_RESIDENT_NT", resident_force_NT, 256, 1024, "threads per workgroup: 256, 512, 768 or 1024 (unset: resident_pick)"),
    KNOB_I("LUTLDPC_RESIDENT_U", resident_U, 1, 4, "frames per lane step of the variable items: 1, 2 or 4 (unset: generator's choice)"),
    KNOB_F("LUTLDPC_RESIDENT_XCD", resident_xcd, "1: workgroup ids remapped so that neighbours share an XCD"),
    KNOB_F("LUTLDPC_RESIDENT_FM", resident_fm, "1: the kernel reads / writes the caller's frame-major buffers itself; 0: always through the row layout"),
    KNOB_F("LUTLDPC_RESIDENT_FLAG_REDUCE", resident_flag_reduce, "wave-reduced exit-test flags (unset: small trees only, resident_spec)"),
    KNOB_F("LUTLDPC_RESIDENT_CN_PERSISTENT", resident_cn_persistent, "check items keep their LDS addresses in registers (unset: where registers allow, resident_spec)"),
    KNOB_I("LUTLDPC_RESIDENT_WAVES_EU", resident_waves_eu, 0, 8, "amdgpu_waves_per_eu of the generated kernel (0: none)"),
    // ---- debugging
    KNOB_F("LUTLDPC_VALIDATE", validate, "1: the class parameters of every per-class launch checked against the allocation sizes (fused roles always are), stream synchronised after every launch so that a device fault names ONE launch; no graph replay"),
    KNOB_F("LUTLDPC_DEBUG_ADDR", debug_addr, "1: print where the row buffers landed (tools/config4_place_ab.sh)"),
};
#undef KNOB_F
#undef KNOB_I
#undef KNOB_R

static void read_knobs(Options &o) {
    for (const Knob &k : kKnobs) {
        const char *e = getenv(k.name);
        if (!e) continue;
        if (k.type == FLAG) o.*k.i = atoi(e) ? 1 : 0;
        else if (k.type == INT) { const int v = atoi(e); if (v >= k.lo && v <= k.hi) o.*k.i = v; }
        else { const double v = atof(e); if (v >= k.lo && (k.type == REAL ? v <= k.hi : v < k.hi)) o.*k.r = v; }
    }
    // what a range cannot say
    if (o.nodes_per_wave_cn == 0) o.nodes_per_wave_cn = o.nodes_per_wave;
    o.use_resident = o.use_resident >= 2 ? 2 : o.use_resident ? 1 : 0;
    if (o.resident_force_NT % 256) o.resident_force_NT = 0;
    if (o.resident_U == 3) o.resident_U = 0;
    if (o.validate) o.use_graph = 0;
    o.compact_margin = (float)o.compact_margin; o.compact_min_share = (float)o.compact_min_share;     // the kernel takes floats
}

lutldpc_decoder::~lutldpc_decoder() {
    if (device < 0) return;
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    drop_graphs();
    for (auto &e : ev_live) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    for (auto &e : ev_pool) (void)hipEventDestroy(e);
}

// ----------------------------------------------------------------------------- decode entries
// frame-major labels of B frames in d_in_cha / d_in_msg (labels_from_host) -> decided bits and iteration codes on the host.
// decode_device leaves the bits in the staging buffer in either of its branches; synchronises.  The dumps of a traced decode
// ([B][E] each, trace_dump) leave through the same buffer before the bits do: it is sized for them here, where its pointer is taken.
static int decode_staged_labels(lutldpc_decoder *d, int B, uint8_t *out_bits, int32_t *out_iters) {
    const size_t n = (size_t)B * (size_t)d->nvar;
    HIP_TRY(d->d_out_bits.alloc(d->trace.level > 1 ? (size_t)B * (size_t)d->E : n));
    int rc = decode_device(d, d->d_in_cha.p, d->d_in_msg.p, B, d->d_out_bits.p);
    if (rc || (rc = copy_to_host(d, out_bits, d->d_out_bits.p, n)) || (rc = iters_to_host(d, out_iters, B))) return rc;
    HIP_TRY(hipStreamSynchronize(d->stream));
    return LUTLDPC_OK;
}

// clears the trace sink of a handle on every way out of a traced decode (as CountedScope of decoder_stats.hip)
struct TraceScope {
    lutldpc_decoder *d;
    explicit TraceScope(lutldpc_decoder *d_) : d(d_) {}
    ~TraceScope() { d->trace = lutldpc_decoder::Trace(); }
};

#pragma GCC visibility pop

// =============================================================================== C-ABI
extern "C" {

const char *lutldpc_last_error(void) { return g_err.c_str(); }
// used by the host mirror (host_capi.cpp) to report through the same channel
void lutldpc_set_last_error(const char *msg) { g_err = msg ? msg : ""; }
const char *lutldpc_version(void) { return "lut_ldpc_amd 0.1 gfx950"; }

int lutldpc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int lutldpc_decoder_create(int nvar, int nchk, const int32_t *dv, const int32_t *dc, const int32_t *cn_msg_idx,
                           int Nq_Cha, const int32_t *Nq_Msg, const uint8_t *reuse_vec, int max_iters,
                           int min_lut, const char *var_trees_txt, const char *chk_trees_txt, int device,
                           lutldpc_decoder **out) {
    if (!out) return fail(LUTLDPC_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (nvar <= 0 || nchk <= 0 || !dv || !dc || !cn_msg_idx || !Nq_Msg || !reuse_vec || max_iters < 1 || !var_trees_txt)
        return fail(LUTLDPC_ERR_ARG, "missing or non-positive argument");
    if (Nq_Cha < 2 || Nq_Cha > 128 || (Nq_Cha & 1)) return fail(LUTLDPC_ERR_ARG, "Nq_Cha must be even and in [2,128]");
    for (int i = 0; i < max_iters; i++)
        if (Nq_Msg[i] < 2 || Nq_Msg[i] > 128 || (Nq_Msg[i] & 1)) return fail(LUTLDPC_ERR_ARG, "Nq_Msg entries must be even and in [2,128]");
    // src/LDPC_Code_LUT.cpp:122
    if (reuse_vec[0] || reuse_vec[max_iters - 1]) return fail(LUTLDPC_ERR_ARG, "first and last iteration are exempt from tree reuse");
    std::unique_ptr<lutldpc_decoder> d(new lutldpc_decoder);
    d->nvar = nvar; d->nchk = nchk;
    d->dv.assign(dv, dv + nvar); d->dc.assign(dc, dc + nchk);
    long long ev = 0, ec = 0;
    for (int v = 0; v < nvar; v++) { if (dv[v] < 1 || dv[v] > 255) return fail(LUTLDPC_ERR_ARG, "variable degree outside [1,255]"); ev += dv[v]; }
    for (int c = 0; c < nchk; c++) { if (dc[c] < 1 || dc[c] > 255) return fail(LUTLDPC_ERR_ARG, "check degree outside [1,255]"); ec += dc[c]; }
    if (ev != ec || ev > (1ll << 30)) return fail(LUTLDPC_ERR_ARG, "sum(dv) != sum(dc)");
    d->E = (int)ev;
    d->cn_msg_idx.assign(cn_msg_idx, cn_msg_idx + d->E);
    d->vn_ptr.resize((size_t)nvar + 1); d->cn_ptr.resize((size_t)nchk + 1);
    for (int v = 0; v < nvar; v++) d->vn_ptr[(size_t)v + 1] = d->vn_ptr[(size_t)v] + dv[v];
    for (int c = 0; c < nchk; c++) d->cn_ptr[(size_t)c + 1] = d->cn_ptr[(size_t)c] + dc[c];
    {   // every edge must appear exactly once; derive chk_equ_idx (VN of each check edge)
        d->edge_vn.resize((size_t)d->E);
        for (int v = 0; v < nvar; v++) for (int e = d->vn_ptr[(size_t)v]; e < d->vn_ptr[(size_t)v + 1]; e++) d->edge_vn[(size_t)e] = v;
        std::vector<uint8_t> seen((size_t)d->E, 0);
        d->cn_vn.resize((size_t)d->E);
        for (int k = 0; k < d->E; k++) {
            int e = cn_msg_idx[k];
            if (e < 0 || e >= d->E || seen[(size_t)e]) return fail(LUTLDPC_ERR_ARG, "cn_msg_idx is not a permutation of the edges");
            seen[(size_t)e] = 1;
            d->cn_vn[(size_t)k] = d->edge_vn[(size_t)e];
        }
    }
    if ((uint64_t)d->E * kRowBytes >= (1ull << 32) || (uint64_t)nvar * kRowBytes >= (1ull << 32))
        return fail(LUTLDPC_ERR_UNSUPPORTED, "code too large: the rows of one frame group must stay below 4 GiB");
    build_classes(d->dv, d->vclass);
    build_classes(d->dc, d->cclass);
    d->Nq_Cha = Nq_Cha; d->Nq_Msg.assign(Nq_Msg, Nq_Msg + max_iters);
    d->max_iters_created = d->max_iters = max_iters; d->psc = 1; d->pisc = 0; d->min_lut = min_lut ? 1 : 0;
    d->iter_set.resize((size_t)max_iters);
    { int cum = 0; for (int i = 0; i < max_iters; i++) { cum += reuse_vec[i] ? 0 : 1; d->iter_set[(size_t)i] = cum - 1; } }
    std::string err;
    if (!parse_tree_array(var_trees_txt, d->var_trees, err)) return fail(LUTLDPC_ERR_PARSE, "var_trees_txt: " + err);
    if (!d->min_lut) {
        if (!chk_trees_txt || !parse_tree_array(chk_trees_txt, d->chk_trees, err)) return fail(LUTLDPC_ERR_PARSE, "chk_trees_txt: " + err);
    }
    read_knobs(d->opt);
    d->pack = 2;
    if (Nq_Cha > 16 || d->opt.pack == 1) d->pack = 1;
    for (int i = 0; i < max_iters; i++) if (Nq_Msg[i] > 16) d->pack = 1;
    int rc = compile_all(d.get());
    if (rc) return rc;
    d->skew_ok = skew_eligible(d.get());
    {
        int max_cn = 0, max_vn = 0;
        for (auto &c : d->cclass) max_cn = std::max(max_cn, c.deg);
        for (auto &c : d->vclass) max_vn = std::max(max_vn, c.deg);
        d->fused_bucket_id = std::max(0, fused_bucket(max_vn, max_cn));
        const int v = d->opt.fused_bucket_min;             // can only widen the bucket
        if (v >= 0 && fused_bucket_rank(v) > fused_bucket_rank(d->fused_bucket_id)) d->fused_bucket_id = v;
    }
    d->device = device;
    if (device >= 0) { rc = upload_static(d.get()); if (rc) return rc; }
    d->resident_ok = resident_eligible(d.get());
    make_describe(d.get());
    *out = d.release();
    return LUTLDPC_OK;
}

int lutldpc_decoder_destroy(lutldpc_decoder *d) {
    if (!d) return LUTLDPC_OK;
    delete d;
    return LUTLDPC_OK;
}

int lutldpc_decoder_set_exit_conditions(lutldpc_decoder *d, int max_iters, int psc, int pisc) {
    if (!d) return fail(LUTLDPC_ERR_ARG, "NULL decoder");
    if (max_iters < 1 || max_iters > d->max_iters_created) return fail(LUTLDPC_ERR_ARG, "max_iters outside [1, value at creation]");
    if (!d->tree_set(TT_DEC, d->iter_set[(size_t)(max_iters - 1)])->valid)
        return fail(LUTLDPC_ERR_ARG, "the tree set of iteration max_iters-1 is not a decision tree set");
    d->max_iters = max_iters; d->psc = psc ? 1 : 0; d->pisc = pisc ? 1 : 0;
    return LUTLDPC_OK;
}

int lutldpc_decoder_decode_batch_device(lutldpc_decoder *d, const uint8_t *d_cha, const uint8_t *d_msg0, int B,
                                        uint8_t *d_out_bits, int32_t *d_out_iters, int sync) {
    if (!d || !d_cha || !d_msg0 || !d_out_bits || !d_out_iters) return fail(LUTLDPC_ERR_ARG, "NULL argument");
    int rc = batch_entry(d, B);
    if (rc || (rc = decode_device(d, d_cha, d_msg0, B, d_out_bits))) return rc;
    HIP_TRY(hipMemcpyAsync(d_out_iters, d->d_iters.p, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToDevice, d->stream));
    if (sync) HIP_TRY(hipStreamSynchronize(d->stream));
    return LUTLDPC_OK;
}

int lutldpc_decoder_decode_batch(lutldpc_decoder *d, const uint8_t *cha, const uint8_t *msg0, int B, uint8_t *out_bits, int32_t *out_iters) {
    if (!d || !cha || !msg0 || !out_bits || !out_iters) return fail(LUTLDPC_ERR_ARG, "NULL argument");
    int rc = batch_entry(d, B);
    if (rc || (rc = labels_from_host(d, cha, msg0, B, (size_t)d->nvar))) return rc;
    return decode_staged_labels(d, B, out_bits, out_iters);
}

// lut_decode of a small batch with the message dumps of output_verbosity = level (2: initial + after every variable update,
// 3: after every check update as well): trace[dump][B][E] label bytes in the reference's print order, n_dumps = 1 + I * (level - 1).
int lutldpc_decoder_decode_batch_trace(lutldpc_decoder *d, const uint8_t *cha, const uint8_t *msg0, int B, int level, uint8_t *out_bits, int32_t *out_iters,
                                       uint8_t *trace, int64_t trace_cap, int32_t *n_dumps) {
    if (!d || !cha || !msg0 || !out_bits || !out_iters || !trace) return fail(LUTLDPC_ERR_ARG, "NULL argument");
    if (level < 2 || level > 3) return fail(LUTLDPC_ERR_ARG, "trace level must be 2 or 3");
    int rc = batch_entry(d, B);
    if (rc) return rc;
    if (B > 4096) return fail(LUTLDPC_ERR_ARG, "the message trace is a debug path: 1..4096 frames");
    const int64_t need = (int64_t)(1 + d->max_iters * (level - 1)) * B * d->E;
    if (trace_cap < need) return fail(LUTLDPC_ERR_ARG, "trace buffer too small: " + std::to_string(need) + " bytes needed");
    TraceScope scope(d);
    d->trace.level = level; d->trace.host = trace; d->trace.cap = (size_t)trace_cap; d->trace.n = 0; d->trace.B = B;
    if ((rc = labels_from_host(d, cha, msg0, B, (size_t)d->nvar)) == LUTLDPC_OK) rc = decode_staged_labels(d, B, out_bits, out_iters);
    if (n_dumps) *n_dumps = d->trace.n;
    return rc;
}

void *lutldpc_decoder_stream(lutldpc_decoder *d) { return d ? (void *)d->stream.s : nullptr; }

int lutldpc_decoder_set_profiling(lutldpc_decoder *d, int enable) {
    if (!d) return fail(LUTLDPC_ERR_ARG, "NULL decoder");
    if (!enable && d->device >= 0) prof_fold(d);
    d->profiling = enable != 0;
    return LUTLDPC_OK;
}
int lutldpc_decoder_get_profile(lutldpc_decoder *d, int kind, double *total_ms, int64_t *launches) {
    if (!d || kind < 0 || kind >= LUTLDPC_K_COUNT) return fail(LUTLDPC_ERR_ARG, "bad kind");
    if (d->device >= 0) prof_fold(d);
    if (total_ms) *total_ms = d->prof_ms[kind];
    if (launches) *launches = d->prof_n[kind];
    return LUTLDPC_OK;
}
int lutldpc_decoder_reset_profile(lutldpc_decoder *d) {
    if (!d) return fail(LUTLDPC_ERR_ARG, "NULL decoder");
    if (d->device >= 0) prof_fold(d);
    for (int i = 0; i < LUTLDPC_K_COUNT; i++) { d->prof_ms[i] = 0; d->prof_n[i] = 0; }
    return LUTLDPC_OK;
}
int64_t lutldpc_decoder_device_bytes(lutldpc_decoder *d) {
    if (!d) return 0;
    return (int64_t)(d->d_msgs.bytes() + d->d_cha_t.bytes() + d->d_msg0_t.bytes() + d->d_hard.bytes() + d->d_state.bytes() + d->d_vfail.bytes() +
                     d->d_iters.bytes() + d->d_in_cha.bytes() + d->d_in_msg.bytes() + d->d_out_bits.bytes() + d->d_host_in.bytes() +
                     d->d_ops.bytes() + d->d_tables.bytes() + d->d_cn_vn.bytes());
}
const char *lutldpc_decoder_describe(lutldpc_decoder *d) { return d ? d->describe.c_str() : ""; }

// kind + 32 (checks): the program over full labels the generated check kernels run (chk_full_label_program)
static const Program *find_prog(lutldpc_decoder *d, int kind, int set, int cls) {
    const bool full = kind == TT_CHK + 32;
    const TreeClassPlan *c = d->tree_class(full ? TT_CHK : kind, set, cls);
    if (!c || (full && c->full.tab.bytes == 0)) return nullptr;
    return full ? &c->full.prog : &c->base.prog;
}
int lutldpc_selftest_program_eval(lutldpc_decoder *d, int kind, int set, int cls, const int32_t *in, int n_in, int32_t *out, int n_out) {
    if (!d || !in || !out) return fail(LUTLDPC_ERR_ARG, "NULL argument");
    const Program *p = find_prog(d, kind, set, cls);
    if (!p) return fail(LUTLDPC_ERR_ARG, "no such program");
    if (n_in != p->n_in || n_out != p->n_out) return fail(LUTLDPC_ERR_ARG, "program arity mismatch");
    if (!eval_program(*p, in, out)) return fail(LUTLDPC_ERR_ARG, "input label outside its alphabet");
    return LUTLDPC_OK;
}
int lutldpc_selftest_program_stats(lutldpc_decoder *d, int kind, int set, int cls, int32_t *n_ops, int32_t *n_ops_naive, int32_t *n_slots) {
    if (!d) return fail(LUTLDPC_ERR_ARG, "NULL decoder");
    const Program *p = find_prog(d, kind, set, cls);
    if (!p) return fail(LUTLDPC_ERR_ARG, "no such program");
    if (n_ops) *n_ops = (int32_t)p->ops.size();
    if (n_ops_naive) *n_ops_naive = p->n_ops_naive;
    if (n_slots) *n_slots = p->n_slots;
    return LUTLDPC_OK;
}

// a generated source handed to the caller: optionally run through hiprtc first (no device needed), copied when cap suffices
static int64_t give_source(const std::string &src, char *buf, int64_t cap, int compile) {
    if (compile) {
        std::vector<char> code; std::string log;
        if (!jit_compile(src, code, log)) return fail(LUTLDPC_ERR_HIP, "hiprtc: " + log.substr(0, 4000));
    }
    if (buf && cap > (int64_t)src.size()) std::memcpy(buf, src.c_str(), src.size() + 1);
    return (int64_t)src.size() + 1;
}

int64_t lutldpc_selftest_jit_source(lutldpc_decoder *d, int kind, int set, int cls, char *buf, int64_t cap, int compile) {
    if (!d) return fail(LUTLDPC_ERR_ARG, "NULL decoder");
    const Program *p = find_prog(d, kind, set, cls);
    if (!p) return fail(LUTLDPC_ERR_ARG, "no such program");
    std::string src, err;
    if (!jit_class_source(d, kind, (size_t)set, (size_t)cls, src, err)) return fail(LUTLDPC_ERR_UNSUPPORTED, err);
    return give_source(src, buf, cap, compile);
}

// Source of the LDS-resident decode kernel for a batch of G frame groups (jit_resident.hpp); compile != 0 also runs hiprtc (no
// device needed).  info (optional, 3 ints): sets per workgroup, threads per workgroup, LDS bytes.  Works on host-only handles.
int64_t lutldpc_selftest_resident_source(lutldpc_decoder *d, int G, char *buf, int64_t cap, int compile, int32_t *info) {
    if (!d || G < 1) return fail(LUTLDPC_ERR_ARG, "NULL decoder / bad G");
    int S = 0, NT = 0, lds = 0;
    if (!resident_pick(d, G, S, NT, lds)) return fail(LUTLDPC_ERR_UNSUPPORTED, "resident decoder: the code does not fit the LDS");
    std::string src, err;
    if (!jit_resident_source(resident_spec(d, S, NT), src, err)) return fail(LUTLDPC_ERR_UNSUPPORTED, "resident decoder: " + err);
    if (info) { info[0] = S; info[1] = NT; info[2] = lds; }
    return give_source(src, buf, cap, compile);
}

}  // extern "C"
