// decoder_state.hpp -- private state of the decode path: the handle behind include/lut_ldpc_hip.h, its device buffers, the
// error / launch macros and the functions that cross the borders of the decoder_*.hip units.  Not installed; no kernel is
// defined here (every kernel has ONE home unit, the others call that unit's host launcher).
//
//   decoder.hip            C-ABI: create (knob table) / destroy / exit conditions / decode entries / profiling / describe / selftest
//   decoder_setup.hip      fills the tree plans (TreeClassPlan: every compiled form of a tree, add_forms) and the dense index tables
//                          (NodeClass: where each sits), chain fusion, JIT registry, static uploads
//   decoder_batch.hip      batch buffers, parameter arena, placement search; the entry layer of the batch entries: one guard
//                          (batch_entry), labels in (tiles_from_host / _device), results out (rows_to_host, iters_to_host)
//   decoder_stream.hip     streaming decode: the kernel of every class (pass_kernel), class parameters (the one builder and validator
//                          of ClassParams), one launch per pass and class -- compile-time, generated or interpreter --, decision
//                          pass, graph replay, message trace   (kernels_generic.hpp)
//   decoder_skew.hip       skewed two-half pipeline through pass_fused_kernel, compaction                     (kernels_compact.hpp)
//   decoder_resident.hip   LDS-resident decoder (jit_resident.hpp)
//   decoder_frontend.hip   Monte-Carlo front end: channel sampler, error counters, sim_batch and sample_labels   (kernels_frontend.hpp)
//   decoder_encode.hip     the generator record (dense or sparse), information bits -> code bits, the sent-bit rows of a batch
//                          (from the encoder or from host bytes), C-ABI   (kernels_encode.hpp, kernels_encode_sparse.hpp)
//   decoder_stats.hip      message-label histograms per dump: edge groups, the counted decode, C-ABI   (kernels_stats.hpp)
//   decoder_events.hip     failed frames captured on the device: weights, selection, sorted error / syndrome lists, C-ABI   (kernels_events.hpp)
//   decoder_layout.hip     frame-major <-> rows: labels in (bytes / nibbles), labels out, decided bits out                  (kernels_layout.hpp)
//   decoder_packed.hip     packed label input and bit-packed output of the host-side batch decode, C-ABI
//   decoder_llr.hip        float64 / float32 / float16 / int8 soft values from host or device memory into both row sets, C-ABI of both LLR entries (kernels_llr.hpp, llr_cells.hpp)
#pragma once
#include "../../../include/lut_ldpc_hip.h"
#include "kernels_common.hpp"
#include "kernels_fast.hpp"
#include "kernels_frontend.hpp"     // FrontEnd, NodeClassTable
#include "lut_program.hpp"
#include "jit.hpp"
#include "jit_resident.hpp"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <sstream>
#include <string>
#include <vector>

namespace lutldpc { LUTLDPC_FAST_LAUNCHERS(extern) }     // instantiated in fast_*.hip / fused_b*.hip

using namespace lutldpc;

#pragma GCC visibility push(hidden)

int fail(int code, const std::string &msg);     // sets the thread's last error (decoder.hip: g_err), returns code

#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return fail(LUTLDPC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));        \
    } while (0)

// device allocation owned by its holder: freed by the destructor, move-only
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t alloc(size_t count) {
        if (count <= n) return hipSuccess;
        release();
        hipError_t e = hipMalloc((void **)&p, count * sizeof(T));
        if (e == hipSuccess) n = count; else p = nullptr;
        return e;
    }
    hipError_t upload(const std::vector<T> &h) {
        hipError_t e = alloc(h.size() ? h.size() : 1);
        if (e != hipSuccess || h.empty()) return e;
        return hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    size_t bytes() const { return n * sizeof(T); }
};

// the decoder's stream; a member declared BEFORE every device buffer, so that it is destroyed after them
struct StreamHolder {
    hipStream_t s = nullptr;
    StreamHolder() = default;
    StreamHolder(const StreamHolder &) = delete;
    StreamHolder &operator=(const StreamHolder &) = delete;
    ~StreamHolder() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
};

struct NodeClass {
    int deg = 0;
    std::vector<int> nodes;     // node ids, ascending
    int tree_class = -1;        // index of the matching tree inside a tree set
    // where the class's dense index tables sit in fast_idx (build_fast_index).  idx_off: variable classes {node id, first edge}
    // per node, check classes the DEG edge ids per node; tidx_off: the same transposed for the LDS-resident decoder ([2][node] /
    // [k][node]).  Checks only: nidx_off / tnidx_off = the NODE of every entry of idx_off / tidx_off (iteration 0 reads the
    // initial-message rows), chain_off = {back, forward} node links of chain fusion (-1: none), npw = checks per wave where
    // the class is chain-rich (0: npw_cn of the degree).  Variables only: red_off / red_n = dense table / count of the nodes NOT
    // updated inside the check pass (-1: the class has no such table)
    int idx_off = 0, tidx_off = 0;
    int nidx_off = 0, tnidx_off = 0, chain_off = -1, npw = 0;
    int red_off = -1, red_n = 0;
};

// One (tree kind, tree set, degree class): every compiled form of its tree (lut_program.hpp: ProgramForm) and the kernels planned
// for it.  A new program form or kernel plan is one more field here.
struct TreeClassPlan {
    ProgramForm base;               // the tree as the reference walks it: interpreter and generated streaming kernels
    int op_off = 0;                 // ... and where its look-ups sit in all_ops
    ProgramForm full;               // checks only: over full labels (chk_full_label_program), for the generated check kernels
    FastClassPlan fast;             // variable / decision classes: balanced-tree plan of the compile-time kernel
    const JitKernel *jit = nullptr; // generated streaming kernel (jit.hpp, build_jit), null = none
};
struct TreeSetPlan {                // valid: the set has trees of this kind (cls is empty otherwise)
    bool valid = false;
    std::vector<TreeClassPlan> cls; // parallel to vclass / cclass
};

#pragma GCC visibility pop

struct lutldpc_decoder {
    // ---- what the user may turn: read once at creation from the environment (decoder.hip: kKnobs holds name, range and
    // meaning of every one; DESIGN.md section 3 lists them)
    struct Options {
        int nodes_per_block = 16;
        int use_fast = 1;
        int pack = 0;                                          // 0 = automatic (lutldpc_decoder::pack), 1 = byte rows
        int nodes_per_wave = 0, nodes_per_wave_cn = 0;         // 0 = derive from the degree (npw_vn / npw_cn)
        int vn_edges_per_wave = 16, cn_edges_per_wave = 0;     // check side: 0 = automatic (cn_epw)
        int first_from_nodes = 1;
        int use_jit = 1;
        int chk_full_labels = 1;
        int use_chain = 1;
        int use_resident = 1, resident_force_S = 0, resident_force_NT = 0, resident_U = 0, resident_xcd = 1, resident_fm = 1;
        int resident_flag_reduce = -1, resident_cn_persistent = -1, resident_waves_eu = 0;      // -1 = automatic (resident_spec)
        int place_candidates = 16;
        int use_compact = -1, compact_first = 8, compact_every = 0;             // use: -1 = automatic, every: 0 = automatic
        double compact_margin = 1.0, compact_min_share = 0.35;
        int use_graph = 1;                                     // also cleared by decode_tiles when a capture fails
        int fused_prio = 0;
        double tail_front = 0.25;
        int skew = 1;
        int late_hard = 1;
        int validate = 0;
        int fused_bucket_min = -1;                             // applied after compile_all (lutldpc_decoder_create)
        int debug_addr = 0;
    } opt;
    // ---- code
    int nvar = 0, nchk = 0, E = 0;
    std::vector<int> dv, dc, cn_msg_idx, vn_ptr, cn_ptr, cn_vn;
    std::vector<NodeClass> vclass, cclass;
    // ---- decoder parameters
    int Nq_Cha = 0, max_iters_created = 0, max_iters = 0, psc = 1, pisc = 0, min_lut = 1;
    std::vector<int> Nq_Msg, iter_set;         // iter_set = cumsum(reuse == 0) - 1
    TreeArray var_trees, chk_trees;
    // ---- programs, launch plans and kernels of every tree: [TT_VAR | TT_CHK | TT_DEC][set].  Read through the three accessors
    // below, which answer nullptr outside the ranges (a set without trees of that kind has no classes); nothing else indexes it.
    std::vector<TreeSetPlan> tree_plans[3];
    const TreeSetPlan *tree_set(int kind, int set) const {
        return kind >= 0 && kind < 3 && set >= 0 && (size_t)set < tree_plans[kind].size() ? &tree_plans[kind][(size_t)set] : nullptr;
    }
    const TreeClassPlan *tree_class(int kind, int set, int cls) const {
        const TreeSetPlan *s = tree_set(kind, set);
        return s && cls >= 0 && (size_t)cls < s->cls.size() ? &s->cls[(size_t)cls] : nullptr;
    }
    // the form a generated check kernel runs: over full labels where that form exists, else (sign, magnitude) as the reference
    const ProgramForm *chk_form(int set, int cls) const {
        const TreeClassPlan *c = tree_class(TT_CHK, set, cls);
        if (!c) return nullptr;
        return c->full.tab.bytes > 0 ? &c->full : &c->base;
    }
    TreeSetPlan *tree_set(int kind, int set) { return const_cast<TreeSetPlan *>(const_cast<const lutldpc_decoder *>(this)->tree_set(kind, set)); }
    TreeClassPlan *tree_class(int kind, int set, int cls) { return const_cast<TreeClassPlan *>(const_cast<const lutldpc_decoder *>(this)->tree_class(kind, set, cls)); }
    std::vector<Op> all_ops;
    std::vector<uint8_t> all_tables;
    // dense per-class index tables of the pass kernels (no pointer chasing, scalar loads); NodeClass says where each sits
    std::vector<int32_t> fast_idx;
    int chain_vclass = -1, n_chain_nodes = 0;   // chain fusion (build_fast_index): the degree-2 class, nodes updated inside the check pass
    std::vector<uint8_t> chain_internal;    // 1 = variable node updated inside the check pass (build_fast_index)
    std::vector<int32_t> edge_vn;           // variable node of every edge (set at creation; chain_hard_kernel reads the device copy)
    int pack = 1;               // 2: nibble rows (all alphabets <= 16 labels and opt.pack = 0), 1: byte rows
    bool skew_ok = false;       // every class of every set has a case in the fused kernel
    int fused_bucket_id = 0;    // degree bucket of the fused kernel (kernels_fast.hpp: kFusedVnDeg / kFusedCnDeg)
    bool resident_ok = false;   // the code can be decoded out of LDS (resident_eligible)
    // ---- device.  The stream comes first: members are destroyed in reverse order, every buffer below goes before it.
    int device = -1;
    StreamHolder stream;
    DevBuf<int32_t> d_vn_ptr, d_cn_ptr, d_cn_vn, d_fast_idx;
    DevBuf<Op> d_ops;
    DevBuf<uint8_t> d_tables;
    DevBuf<uint8_t> d_chain_internal;
    DevBuf<int32_t> d_edge_vn;
    // batch buffers
    int Bcap = 0;
    DevBuf<uint8_t> d_msgs, d_cha_t, d_msg0_t, d_hard, d_state, d_vfail;
    DevBuf<int32_t> d_iters;
    DevBuf<uint8_t> d_in_cha, d_in_msg, d_out_bits;   // frame-major staging for the host entry points
    DevBuf<uint32_t> d_out_words;                     // decode_batch_packed: [B][ceil(out_count/32)] decided bits, one each (encode_packed: codeword bits)
    DevBuf<uint64_t> d_host_in;                       // raw host input of any element type, staged as it came: the soft values of the LLR entries, the information words of encode_packed
    DevBuf<uint8_t> d_codewords;                      // upload staging of sent_rows_from_host; no kernel but its conversion reads it
    DevBuf<int32_t> d_stats;
    // The systematic generator of the device encoder (decoder_encode.hip), R parity rows over K information bits, in the form it
    // was set in; a setter builds a complete record and moves it here, which frees the buffers of the one it replaces.
    // dense (lutldpc_decoder_set_generator, kernels_encode.hpp): the rows as whole 32-row tiles of W32p = 4*ceil(K/128) dwords.
    // sparse (lutldpc_decoder_set_sparse_generator, kernels_encode_sparse.hpp): the arrays of lut_ldpc::SparsePacked on the device,
    // Rp solve positions in whole blocks.
    struct Generator {
        enum Form { NONE = 0, DENSE, SPARSE } form = NONE;
        int K = 0, R = 0;
        struct { int W32p = 0; DevBuf<uint32_t> A; } dense;
        struct Sparse {
            int Rp = 0, depth = 0, block = 0;
            long long terms = 0;
            DevBuf<int32_t> a_ptr, a_cols, order, e_ptr, e_cols;
            DevBuf<uint64_t> inv;
        } sparse;
    } gen;
    // Per-node channel classes of the sampler (lutldpc_decoder_set_node_channels, decoder_frontend.hip): n classes (0 = none set),
    // their LDS images (n NodeClassTable of kernels_frontend.hpp, bucket index included) and the class byte of every node on the
    // device (allocated once for 16 classes, written in place by every set); nodes[c] = nodes of class c, for describe().
    struct NodeChannels {
        int n = 0;
        std::vector<int> nodes;
        DevBuf<uint64_t> tables;
        DevBuf<uint8_t> node_class;
    } node_channels;
    // d_sent: the sent-bit rows of a batch; d_enc_rows: the bit rows encode_packed works on with the sparse form (its own: no entry
    // of a decode reads or writes them)
    DevBuf<uint8_t> d_sent, d_enc_rows;
    // compaction of the surviving frames (kernels_compact.hpp)
    DevBuf<int32_t> d_frame_of, d_perm, d_tmp3, d_ctl, d_slot_of, d_iters_tmp;
    DevBuf<int32_t> d_grp;                           // per frame group: every frame failed the probe of the test on the channel decisions
    // Parameter structures of the per-class / generic / sampler kernels live in DEVICE memory (kernel arguments stay <= 128 bytes,
    // kernels_common.hpp: launch_k): a small arena keyed by content.  The first decode of a shape runs as plain launches and
    // uploads what it needs; the captured second run finds every structure there already.
    struct ParamArena {
        std::map<std::string, size_t> off_of;        // content -> byte offset (the key's bytes are the host copy the upload reads)
        std::vector<DevBuf<uint8_t>> chunks;
        std::vector<size_t> chunk_base;
        size_t used = 0, cap = 0;
        void clear() { chunks.clear(); chunk_base.clear(); off_of.clear(); used = cap = 0; }
    } params;
    // message dumps of output_verbosity >= 2 (src/LDPC_Code_LUT.cpp:292-298,311-317,331-337): a small-batch debug path -- per-class
    // streaming launches, the edge rows copied out after the edge initialisation, (level > 2) every check pass and every
    // variable pass.  host: [dump][B][E] bytes, dumps in the reference's print order.
    // The sink of a dump is either that host copy, or (hist != nullptr) a histogram: the labels of the dump are counted on the device
    // into hist[dump][group][sent bit][n_labels] 64-bit totals, nothing is copied (decoder_stats.hip: hist_dump) -- any batch size.
    // sent: sent-bit rows or null (all-zero codeword); last_dump[f]: how many dumps of frame f are counted.
    struct Trace {
        int level = 0; uint8_t *host = nullptr; size_t cap = 0; int n = 0; int B = 0;
        unsigned long long *hist = nullptr; const uint8_t *sent = nullptr; const int32_t *last_dump = nullptr; int n_labels = 0, n_dumps = 0;
    };
    Trace trace;
    // edge grouping of the histograms (lutldpc_decoder_set_edge_groups): the edges sorted by group, where every group's run
    // begins, and the runs cut into chunks {first, count, group} of hist_chunk_edges edges (decoder_stats.hip:
    // upload_edge_groups; 0 = not cut / uploaded yet).  hist_edges empty = never set (one group)
    int hist_groups = 1, hist_chunk_edges = 0;
    std::vector<int32_t> hist_edges, hist_run, hist_chunks;
    DevBuf<int32_t> d_hist_edges, d_hist_chunks, d_last_dump;
    DevBuf<unsigned long long> d_hist;
    // capture of failed frames (decoder_events.hip; allocated by the first capture call, never by a plain decode): per-frame
    // weights [bpad][4], slot of every frame, {selected, stored}, the records and lists of the kept frames, the byte counts of
    // every node / check run [run][bpad] with their prefix sums per kept frame [run][slots], the two profiles
    struct Events {
        DevBuf<int32_t> frame_w, slot_of, counters, records, positions, checks, off_n, off_c;
        DevBuf<uint8_t> cnt_n, cnt_c;
        DevBuf<unsigned long long> node_errors, check_fails;
    } ev;
    // LDS-resident decoder (jit_resident.hpp): codes whose edge messages fit the LDS of a compute unit are decoded by ONE generated
    // kernel per decode -- all iterations inside, no HBM traffic between the labels and the decided bits.
    struct ResidentPlan { int S = 0, NT = 0, lds = 0; const JitKernel *k = nullptr; };
    std::map<int, ResidentPlan> resident_plans;       // by frame groups
    std::string resident_log;
    // tree-specialised kernels for shapes the compile-time path does not cover (jit.hpp); the loaded kernels live in a
    // process-wide registry keyed by device + source text, see jit_registry(): decoders share them and they are never unloaded
    std::string jit_log;                                               // last hiprtc diagnostic (describe())
    // repeated decodes replayed as one hipGraph launch (decode_tiles)
    struct GraphSlot { int seen = 0; hipGraphExec_t exec = nullptr; };
    std::map<std::array<int, 4>, GraphSlot> graphs;       // key {B, psc, pisc, max_iters}
    void drop_graphs() { for (auto &kv : graphs) if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec); graphs.clear(); }
    // specialised kernels: nodes handled by one wave = edges_per_wave / degree (equal work per wave for every degree class); a
    // fixed count when opt.nodes_per_wave[_cn] is set
    int cn_epw() const { return opt.cn_edges_per_wave > 0 ? opt.cn_edges_per_wave : 42; }
    int npw_vn(int deg) const { return opt.nodes_per_wave > 0 ? opt.nodes_per_wave : std::max(1, opt.vn_edges_per_wave / std::max(deg, 1)); }
    int npw_cn(int deg) const { return opt.nodes_per_wave_cn > 0 ? opt.nodes_per_wave_cn : std::max(1, cn_epw() / std::max(deg, 1)); }
    int npw_cn_class(size_t ci) const { return cclass[ci].npw > 0 ? cclass[ci].npw : npw_cn(cclass[ci].deg); }     // chain-rich classes of wide checks get at least 4
    std::string place_info = "null";                  // what the placement search did (decoder_batch.hip: place_rows), JSON
    // launch plan of the skewed pipeline for one (frame groups, psc, max_iters): the roles of every launch in DEVICE memory
    // (the kernel reads them through a pointer), the interleaved item tables, what follows each launch.  Built once, at
    // the first decode of that shape; dropped with the batch buffers (the roles hold strides of the flag buffers).
    struct SkewSlot { int n_roles = 0; size_t role_off = 0; const int32_t *items = nullptr; int nb = 0; int state_half = -1, state_ii = 0; };
    struct SkewPlan { std::vector<SkewSlot> slots; std::vector<ClassParams> h_roles; DevBuf<ClassParams> d_roles; };
    std::map<std::array<int, 3>, std::unique_ptr<SkewPlan>> skew_plans;
    // interleaved item tables, keyed by the role block counts AND the (quantised) share of the timeline each role keeps clear
    std::map<std::pair<std::vector<int>, std::vector<int>>, DevBuf<int32_t>> item_tabs;
    void drop_plans() { skew_plans.clear(); item_tabs.clear(); }
    int tile() const { return kRowBytes * pack; }       // frames per group
    int bpad(int B) const { return (B + tile() - 1) / tile() * tile(); }
    // ---- profiling
    bool profiling = false;
    struct Ev { hipEvent_t a, b; int kind; };
    std::vector<Ev> ev_live;
    std::vector<hipEvent_t> ev_pool;
    double prof_ms[LUTLDPC_K_COUNT] = {0};
    int64_t prof_n[LUTLDPC_K_COUNT] = {0};
    std::string describe;

    lutldpc_decoder() = default;
    lutldpc_decoder(const lutldpc_decoder &) = delete;
    lutldpc_decoder &operator=(const lutldpc_decoder &) = delete;
    // device = -1 (host-only handle): no HIP call.  Otherwise: the device made current, the stream drained, graphs and events
    // destroyed; the members then release every buffer, the stream last.
    ~lutldpc_decoder();
};

#pragma GCC visibility push(hidden)

// LUTLDPC_VALIDATE=1: additionally wait for the launch(es) just issued, so that a device fault is reported by the launch site
// that caused it (function and line), whatever the kernel -- not only the fused ones (no graph capture in that mode)
#define LAUNCH_CHECK()                                                                              \
    do {                                                                                            \
        hipError_t e_ = hipGetLastError();                                                          \
        if (e_ != hipSuccess) return fail(LUTLDPC_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e_)); \
        if (d->opt.validate) {                                                                      \
            e_ = hipStreamSynchronize(d->stream);                                                   \
            if (e_ == hipSuccess) e_ = hipGetLastError();                                           \
            if (e_ != hipSuccess) return fail(LUTLDPC_ERR_HIP, std::string("launch failed on the device (") + __func__ + ":" + std::to_string(__LINE__) + "): " + hipGetErrorString(e_)); \
        }                                                                                           \
    } while (0)

// device copy of a parameter structure (see lutldpc_decoder::ParamArena); nullptr + last error on failure
const void *dev_param_bytes(lutldpc_decoder *d, const void *src, size_t n);
template <class T> const T *dev_param(lutldpc_decoder *d, const T &v) { return static_cast<const T *>(dev_param_bytes(d, &v, sizeof(T))); }
#define DEV_PARAM(var, d, v)                      \
    const auto *var = dev_param((d), (v));        \
    if (!var) return LUTLDPC_ERR_HIP

// instantiate a launch for the decoder's packing
#define PACK_DISPATCH(d, ...)                        \
    do {                                             \
        if ((d)->pack == 2) { constexpr int PK = 2; __VA_ARGS__; } \
        else { constexpr int PK = 1; __VA_ARGS__; }  \
    } while (0)

// ---- profiling (decoder.hip): kernel time by kind, from event pairs around the launches of a scope
hipEvent_t ev_get(lutldpc_decoder *d);
void prof_fold(lutldpc_decoder *d);
struct Timed {
    lutldpc_decoder *d; int kind; hipEvent_t a{}, b{};
    Timed(lutldpc_decoder *d_, int k) : d(d_), kind(k) {
        if (d->profiling) { a = ev_get(d); b = ev_get(d); (void)hipEventRecord(a, d->stream); }
    }
    ~Timed() {
        if (d->profiling) { (void)hipEventRecord(b, d->stream); d->ev_live.push_back({a, b, kind}); }
    }
};
void make_describe(lutldpc_decoder *d);

// ---- decoder_setup.hip
void build_classes(const std::vector<int> &deg, std::vector<NodeClass> &cls);
int compile_all(lutldpc_decoder *d);
int upload_static(lutldpc_decoder *d);
// Process-wide registry of the run-time generated kernels, keyed by device + source text (decoder_setup.hip: jit_registry)
struct JitRegistry { std::mutex mu; std::map<std::string, JitKernel> by_src; };
constexpr size_t kJitRegistryMax = 4096;
JitRegistry &jit_registry();
JitKernel *jit_get(int device, const std::string &src, std::string &log);      // registry look-up, else compile + load + remember
bool jit_class_source(const lutldpc_decoder *d, int kind, size_t s, size_t i, std::string &src, std::string &err);

// ---- decoder_batch.hip
int ensure_batch(lutldpc_decoder *d, int B);
int check_batch_buffers(const lutldpc_decoder *d, int Bpad);
// The entry layer: what every batch entry of the C-ABI does around decode_tiles.
// The guard, in the order of the header's error contract: NULL handle, B <= 0 (LUTLDPC_ERR_ARG), host-only handle
// (LUTLDPC_ERR_STATE), then the handle's device made current.  device_entry: the same without a batch (set_generator).
// stream: the Philox stream of the entries that sample or encode (lutldpc_check_stream: >= 2^31 is LUTLDPC_ERR_ARG too).
int device_entry(lutldpc_decoder *d);
int batch_entry(lutldpc_decoder *d, int B, uint32_t stream = 0);
// labels in: frame-major labels of B frames -> d_cha_t / d_msg0_t.  labels_from_host uploads them, `stride` bytes per frame, to
// d_in_cha / d_in_msg (msg0 = null: the channel labels alone) and stops there (decode_device decides whether rows are needed),
// tiles_from_host goes on to the rows.
int tiles_from_device(lutldpc_decoder *d, const uint8_t *d_cha, const uint8_t *d_msg0, int B);
int labels_from_host(lutldpc_decoder *d, const uint8_t *cha, const uint8_t *msg0, int B, size_t stride);
int tiles_from_host(lutldpc_decoder *d, const uint8_t *cha, const uint8_t *msg0, int B);
// results out, asynchronous on the decoder's stream.  Rows are staged through d_out_bits (copies on one stream are ordered: a
// caller may fetch several row sets one after the other).
int copy_to_host(lutldpc_decoder *d, void *host_dst, const void *src, size_t bytes);
int rows_to_host(lutldpc_decoder *d, const uint8_t *rows, uint8_t *host_dst, int B, int n_rows = 0);      // n_rows = 0: nvar
int iters_to_host(lutldpc_decoder *d, int32_t *dst, int B);                                                // d_iters of the last decode_tiles
// the packed entries: LUTLDPC_ERR_ARG unless decided / codeword bits first .. first + count - 1 lie inside [0, nvar)
int check_out_window(const lutldpc_decoder *d, int first, int count);
// decided bits first .. first + count - 1 of the last decode_tiles -> words[B][ceil(count/32)], one bit each: written in place
// where `words` is device memory, else staged through d_out_words
int bits_to_caller(lutldpc_decoder *d, uint32_t *words, bool on_device, int B, int first, int count);

// ---- decoder_stream.hip (home of the kernels of kernels_generic.hpp)
hipError_t preload_stream_kernels();
// frames f0 .. f1-1 (both multiples of 256); default: the whole padded batch
// `sel`: which of the two flag buffers the exit test reads and clears (always 0 outside the skewed pipeline)
int launch_state(lutldpc_decoder *d, int B, int Bpad, int mode, int value, int f0 = 0, int f1 = -1, int sel = 0);
bool chain_active(const lutldpc_decoder *d, int set);
// The kernel that runs degree class `cls` of a pass of `kind` (TT_VAR, TT_CHK, TT_DEC) with tree set `set` and sign threshold nz
// (ClassParams::nz): the only place that chooses.  Launches, class parameters, describe() and skew_eligible ask here.
enum PassKernel { KERNEL_FAST, KERNEL_GENERATED, KERNEL_INTERPRETER };      // compile-time (kernels_fast.hpp), jit.hpp, kernels_generic.hpp
PassKernel pass_kernel(const lutldpc_decoder *d, int kind, int set, int cls, int nz);
// One degree class of one pass for the frame groups `groups`: complete ClassParams, the only code that assigns their fields.
// skew_ii: the iteration of a role of the skewed pipeline (its flag buffers, chain block, first pass), or kPerClassLaunch for
// a launch of the streaming decode (flag buffer 0, no chain, inputs from the edge rows).
struct HalfRange { int g0, G; };
constexpr int kPerClassLaunch = -1;
ClassParams cn_class_params(const lutldpc_decoder *d, size_t ci, HalfRange groups, int nz, int check, int skew_ii = kPerClassLaunch);
ClassParams lut_cn_class_params(const lutldpc_decoder *d, int set, size_t ci, HalfRange groups, int nz, int check);      // LUT checks: generated kernel or interpreter
ClassParams vn_class_params(const lutldpc_decoder *d, int kind, int set, size_t ci, HalfRange groups, int nz, int check, int write_hard, int skew_ii = kPerClassLaunch);
// the balanced-tree kernel has a case for the class (pass_kernel decides); where it reads the root as packed rows, the plan has them
inline bool fast_covers(const lutldpc_decoder *d, const FastClassPlan &f, int kind, int deg) {
    return d->opt.use_fast && f.ok && deg <= kFastMaxDeg && (!vn_root_rows(kind, d->pack, deg) || f.rows_off >= 0);
}
// the kernel a ClassParams is meant for: its pass, compile-time (min-sum, balanced tables of <= 256 bytes) or one class blob
// (`generated`: the generated kernels and the interpreter), the degrees it has cases for and what the error message calls that limit
struct KernelCases { int tree_kind; bool generated; int max_vn_deg, max_cn_deg; const char *limit; };
// LDS of an interpreter launch (tree_pass_kernel): value slots and staged outputs, one dword per lane each; the class's tables
// follow where the sum stays within 64 KiB
inline int interp_slot_bytes(const Program &p) { return (p.n_slots + p.n_out) * kWave * 4; }
// a ClassParams against the decoder's allocations and the cases of its kernel; `where` opens the error message
int validate_class(const lutldpc_decoder *d, const ClassParams &P, const std::string &where, const KernelCases &k);
inline PassBufs pass_bufs(const lutldpc_decoder *d) {
    return {d->d_msgs.p, d->d_cha_t.p, d->d_hard.p, reinterpret_cast<const uint32_t *>(d->d_state.p), reinterpret_cast<uint32_t *>(d->d_vfail.p), d->d_tables.p,
            d->d_fast_idx.p, d->d_msg0_t.p};
}
bool late_hard_active(const lutldpc_decoder *d, bool skewed, bool *chain_skip);
int launch_late_hard(lutldpc_decoder *d, bool skewed, int g0, int G);
// The frame-major label / bit buffers of a decode_device call (the C-ABI's own layout, [B][nvar] bytes, device), handed down to
// the resident kernel, which reads and writes them itself: no transposes.  No record = rows, as every other caller has them.
struct FrameMajorIO { const uint8_t *cha, *msg0; uint8_t *bits; };
int decode_tiles(lutldpc_decoder *d, int B, const FrameMajorIO *fm = nullptr);
int decode_device(lutldpc_decoder *d, const uint8_t *d_cha, const uint8_t *d_msg0, int B, uint8_t *d_out_bits);

// ---- decoder_skew.hip (home of the kernels of kernels_compact.hpp; pass_fused_kernel through launch_fused)
// Half A = groups [0, GA), half B = [GA, G)
hipError_t preload_compact_kernels();
bool skew_eligible(const lutldpc_decoder *d);
bool compaction_on(const lutldpc_decoder *d, int G);
int compaction_min_groups(const lutldpc_decoder *d);       // smallest batch, in frame groups, that compaction_on accepts (-1: none)
int launch_uncompaction(lutldpc_decoder *d, const HalfRange (&half)[2], int Bpad);
int iterate_skewed(lutldpc_decoder *d, int B, int Bpad, int G);

// ---- decoder_resident.hip
ResidentSpec resident_spec(const lutldpc_decoder *d, int S, int NT);
bool resident_eligible(const lutldpc_decoder *d);
bool resident_pick(const lutldpc_decoder *d, int G, int &S_out, int &NT_out, int &lds_out);
inline bool resident_active(const lutldpc_decoder *d) { return d->resident_ok && d->opt.use_resident; }
int resident_plan_for(lutldpc_decoder *d, int G, lutldpc_decoder::ResidentPlan **out);
int launch_resident(lutldpc_decoder *d, int G, int B, const FrameMajorIO *fm = nullptr);

// ---- decoder_frontend.hip (home of the kernels of kernels_frontend.hpp)
hipError_t preload_frontend_kernels();
// what an entry that takes `cells` samples with: the caller's table where one is given (checked, made into the sampler's image and
// placed in the parameter arena), else the handle's node channels, else the LUTLDPC_ERR_ARG of the table checks for a NULL table
int front_end_of(const lutldpc_channel_cells *cells, lutldpc_decoder *d, FrontEnd &fe);
// sampler -> d_cha_t / d_msg0_t with the front end `fe`; sent_rows: the sent bits as sent-bit rows (device), null = all-zero codeword
int sample_tiles(lutldpc_decoder *d, const FrontEnd &fe, uint64_t seed, uint32_t stream, uint64_t frame0, int B, const uint8_t *sent_rows);
// lutldpc_decoder_sim_batch / _random; req != null: the capture of decoder_events.hip on top (lutldpc_decoder_sim_batch_events)
int sim_batch_impl(lutldpc_decoder *d, const lutldpc_channel_cells *cells, uint64_t seed, uint32_t stream, uint64_t frame0, int B, const uint8_t *codewords,
                   bool device_codewords, int K_info, int32_t *frame_stats, uint8_t *cha_out, uint8_t *bits_out, lutldpc_event_request *req = nullptr);

// ---- decoder_encode.hip (home of the kernels of kernels_encode.hpp and kernels_encode_sparse.hpp)
hipError_t preload_encode_kernels();
// the entries that encode: LUTLDPC_ERR_STATE with the entry's own text unless the handle has a generator
inline int require_generator(const lutldpc_decoder *d, const char *text) { return d->gen.form ? LUTLDPC_OK : fail(LUTLDPC_ERR_STATE, text); }
// random codewords of frames frame0 .. frame0+B-1 -> d_sent (sent-bit rows of bpad(B) frames; pad frames zero)
int encode_tiles(lutldpc_decoder *d, uint64_t seed, uint32_t stream, uint64_t frame0, int B);
// host frame-major codewords of B frames (bytes 0 / 1: bit 0 counts) -> d_codewords (upload staging) -> *rows = d_sent;
// codewords = null: *rows = null, the all-zero codeword
int sent_rows_from_host(lutldpc_decoder *d, const uint8_t *codewords, int B, const uint8_t **rows);
// the sent bits of a batch in their one device form: *rows = d_sent filled by the encoder (device_codewords) or from the caller's
// frame-major bytes (codewords, host), or null = all-zero codeword.  Sampler, error counters, histograms and the capture read it.
int sent_rows_of(lutldpc_decoder *d, const uint8_t *codewords, bool device_codewords, uint64_t seed, uint32_t stream, uint64_t frame0, int B,
                 const uint8_t **rows);

// ---- decoder_stats.hip (home of the kernels of kernels_stats.hpp)
hipError_t preload_stats_kernels();
int hist_dump(lutldpc_decoder *d);           // one dump of a counted decode: the message rows into d->trace.hist (decode_tiles_launch)

// ---- decoder_events.hip (home of the kernels of kernels_events.hpp)
hipError_t preload_events_kernels();
int event_request_check(const lutldpc_event_request *req);                         // LUTLDPC_ERR_ARG for a malformed request
// after decode_tiles of B frames: weights, selection and lists of the batch in d_hard / d_iters into req.  sent_rows: sent-bit
// rows of the batch or null (all-zero codeword); stats: the front end's per-frame counters (device) or null.  Synchronises.
int capture_events(lutldpc_decoder *d, int B, int K_info, const uint8_t *sent_rows, const int32_t *stats, lutldpc_event_request *req);

// ---- decoder_layout.hip (home of the kernels of kernels_layout.hpp)
hipError_t preload_layout_kernels();
// frame-major labels of B frames (device, `stride` bytes per frame, one label per byte or two with `nibbles`) -> rows_a =
// min(label, lim_a) and, with lut_b (device, 256 entries), rows_b = lut_b[label]; rows_b = lut_b = null: one row set
int launch_labels_in(lutldpc_decoder *d, const uint8_t *src, size_t stride, bool nibbles, uint8_t *rows_a, uint8_t *rows_b, const uint8_t *lut_b,
                     int B, int G, int lim_a);
// rows -> frame-major dst[B][rows] (device); rows = 0: nvar
int launch_transpose_out(lutldpc_decoder *d, const uint8_t *src_rows, uint8_t *dst, int B, int G, int rows = 0);
int launch_bits_out(lutldpc_decoder *d, uint32_t *dst, int B, int G, int first, int count);     // a window of d_hard -> dst[B][ceil(count/32)], device

// ---- decoder_llr.hip (home of the kernel of kernels_llr.hpp)
hipError_t preload_llr_kernels();

#pragma GCC visibility pop
