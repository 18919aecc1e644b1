// decoder_setup.hip -- what a decoder is made of at creation: degree classes, compiled tree programs, the dense index tables of
// the specialised kernels (with the chain links), the run-time generated kernels and the static uploads.
#include "decoder_state.hpp"

#pragma GCC visibility push(hidden)

// ----------------------------------------------------------------------------- set-up helpers
void build_classes(const std::vector<int> &deg, std::vector<NodeClass> &cls) {
    std::map<int, std::vector<int>> by;
    for (size_t i = 0; i < deg.size(); i++) by[deg[i]].push_back((int)i);
    cls.clear();
    for (auto &kv : by) { NodeClass c; c.deg = kv.first; c.nodes = kv.second; cls.push_back(std::move(c)); }
}

static void build_fast_index(lutldpc_decoder *d) {
    d->fast_idx.clear();
    for (auto &c : d->cclass) { c.chain_off = -1; c.npw = 0; }
    for (auto &c : d->vclass) {
        c.red_off = -1; c.red_n = 0;
        c.idx_off = (int)d->fast_idx.size();
        for (int v : c.nodes) { d->fast_idx.push_back(v); d->fast_idx.push_back(d->vn_ptr[(size_t)v]); }
    }
    // ---- chain links (kernels_fast.hpp: cn_minsum_body<..., CHAIN>).  A degree-2 variable node whose two checks
    // are neighbours in their degree class AND fall into the same wave (the same run of npw checks) is updated by
    // that wave inside the check pass: both of its incoming messages are in registers there.  back[c] / fwd[c] =
    // the node check c shares with its predecessor / successor in the class list (+1, 0 = none).
    std::vector<int> edge_chk((size_t)d->E, -1), cls_of((size_t)d->nchk, -1), pos_of((size_t)d->nchk, -1);
    for (int c = 0; c < d->nchk; c++)
        for (int k = d->cn_ptr[(size_t)c]; k < d->cn_ptr[(size_t)c + 1]; k++) edge_chk[(size_t)d->cn_msg_idx[(size_t)k]] = c;
    for (size_t ci = 0; ci < d->cclass.size(); ci++)
        for (size_t j = 0; j < d->cclass[ci].nodes.size(); j++) { cls_of[(size_t)d->cclass[ci].nodes[j]] = (int)ci; pos_of[(size_t)d->cclass[ci].nodes[j]] = (int)j; }
    std::vector<int> back((size_t)d->nchk, 0), fwd((size_t)d->nchk, 0);
    std::vector<char> internal((size_t)d->nvar, 0);
    // checks per wave: a class of wide checks whose members are mostly linked by degree-2 nodes (the zigzag of a dual-diagonal
    // code) gets at least four checks per wave, so that three of four links fall inside a wave -- and twelve where the class is
    // large enough to keep 2048 runs per frame group (DVB-S2: 11 of 12 links inside a wave, +0.9 % over six checks per wave;
    // 18 per wave is slower again, tools/env_sweep.sh)
    if (d->opt.use_chain && d->min_lut) {
        std::vector<int> cand(d->cclass.size(), 0);
        for (int v = 0; v < d->nvar; v++) {
            if (d->dv[(size_t)v] != 2) continue;
            const int e0 = d->vn_ptr[(size_t)v], c1 = edge_chk[(size_t)e0], c2 = edge_chk[(size_t)e0 + 1];
            if (c1 < 0 || c2 < 0 || c1 == c2 || cls_of[(size_t)c1] != cls_of[(size_t)c2]) continue;
            if (std::abs(pos_of[(size_t)c1] - pos_of[(size_t)c2]) == 1) cand[(size_t)cls_of[(size_t)c1]]++;
        }
        for (size_t ci = 0; ci < d->cclass.size(); ci++)
            if (2 * cand[ci] >= (int)d->cclass[ci].nodes.size() && d->opt.nodes_per_wave_cn <= 0) {
                const int n = (int)d->cclass[ci].nodes.size();
                d->cclass[ci].npw = std::max(4, d->npw_cn(d->cclass[ci].deg));
                if (d->opt.cn_edges_per_wave <= 0) d->cclass[ci].npw = std::max(d->cclass[ci].npw, std::min(12, n / 2048));
            }
    }
    if (d->opt.use_chain && d->min_lut)
        for (int v = 0; v < d->nvar; v++) {
            if (d->dv[(size_t)v] != 2) continue;
            const int e0 = d->vn_ptr[(size_t)v];
            int c1 = edge_chk[(size_t)e0], c2 = edge_chk[(size_t)e0 + 1];
            if (c1 < 0 || c2 < 0 || c1 == c2 || cls_of[(size_t)c1] != cls_of[(size_t)c2]) continue;
            if (pos_of[(size_t)c1] > pos_of[(size_t)c2]) std::swap(c1, c2);
            const int deg = d->cclass[(size_t)cls_of[(size_t)c1]].deg, npw = d->npw_cn_class((size_t)cls_of[(size_t)c1]);
            if (deg < 2 || deg > fused_max_cn_deg() || pos_of[(size_t)c2] != pos_of[(size_t)c1] + 1 || pos_of[(size_t)c1] / npw != pos_of[(size_t)c2] / npw) continue;
            if (fwd[(size_t)c1] || back[(size_t)c2]) continue;
            fwd[(size_t)c1] = v + 1; back[(size_t)c2] = v + 1; internal[(size_t)v] = 1;
        }
    for (size_t ci = 0; ci < d->cclass.size(); ci++) {
        auto &c = d->cclass[ci];
        c.idx_off = (int)d->fast_idx.size();
        bool any = false;
        for (int cn : c.nodes) {
            std::vector<int> es;
            for (int k = 0; k < c.deg; k++) es.push_back(d->cn_msg_idx[(size_t)(d->cn_ptr[(size_t)cn] + k)]);
            // the order of a check's edges is free (min-sum is symmetric): chain edges go to fixed slots, back = 0, forward = 1
            auto to_slot = [&](int v1, size_t slot) {
                if (!v1) return;
                for (size_t k = 0; k < es.size(); k++)
                    if (es[k] == d->vn_ptr[(size_t)(v1 - 1)] || es[k] == d->vn_ptr[(size_t)(v1 - 1)] + 1) { std::swap(es[k], es[slot]); return; }
            };
            to_slot(back[(size_t)cn], 0); to_slot(fwd[(size_t)cn], 1);
            if (back[(size_t)cn] && fwd[(size_t)cn] && c.deg >= 2) {     // the second swap may have moved the back edge: restore slot 0
                const int vb = back[(size_t)cn] - 1;
                if (es[0] != d->vn_ptr[(size_t)vb] && es[0] != d->vn_ptr[(size_t)vb] + 1) to_slot(back[(size_t)cn], 0);
            }
            for (int e : es) d->fast_idx.push_back(e);
            any = any || back[(size_t)cn] || fwd[(size_t)cn];
        }
        if (any) {
            c.chain_off = (int)d->fast_idx.size();
            for (int cn : c.nodes) { d->fast_idx.push_back(back[(size_t)cn]); d->fast_idx.push_back(fwd[(size_t)cn]); }
        }
    }
    // the node behind every entry of the check classes' edge tables, same order
    for (auto &c : d->cclass) {
        const size_t off = (size_t)c.idx_off, cnt = c.nodes.size() * (size_t)c.deg;
        c.nidx_off = (int)d->fast_idx.size();
        for (size_t j = 0; j < cnt; j++) d->fast_idx.push_back(d->edge_vn[(size_t)d->fast_idx[off + j]]);
    }
    // LDS-resident decoder (jit_resident.hpp): there a LANE owns a node, so the tables are transposed -- [k][node of the class] --
    // and 64 lanes reading entry k of 64 consecutive nodes touch 256 contiguous bytes.  Canonical edge order of the check
    // (ascending variable node, as cn_msg_idx: a CHKTREE consumes its inputs in that order).
    for (auto &c : d->cclass) {
        const size_t n = c.nodes.size();
        c.tidx_off = (int)d->fast_idx.size();
        for (int k = 0; k < c.deg; k++) for (size_t j = 0; j < n; j++) d->fast_idx.push_back(d->cn_msg_idx[(size_t)(d->cn_ptr[(size_t)c.nodes[j]] + k)]);
        c.tnidx_off = (int)d->fast_idx.size();
        for (int k = 0; k < c.deg; k++) for (size_t j = 0; j < n; j++) d->fast_idx.push_back(d->edge_vn[(size_t)d->cn_msg_idx[(size_t)(d->cn_ptr[(size_t)c.nodes[j]] + k)]]);
    }
    for (auto &c : d->vclass) {
        c.tidx_off = (int)d->fast_idx.size();
        for (int v : c.nodes) d->fast_idx.push_back(v);
        for (int v : c.nodes) d->fast_idx.push_back(d->vn_ptr[(size_t)v]);
    }
    // variable passes that follow a chained check pass skip the nodes it already updated
    for (size_t vi = 0; vi < d->vclass.size(); vi++) {
        auto &c = d->vclass[vi];
        if (c.deg != 2) continue;
        c.red_off = (int)d->fast_idx.size();
        for (int v : c.nodes)
            if (!internal[(size_t)v]) { d->fast_idx.push_back(v); d->fast_idx.push_back(d->vn_ptr[(size_t)v]); c.red_n++; }
        d->chain_vclass = (int)vi;
    }
    d->n_chain_nodes = 0;
    for (char x : internal) d->n_chain_nodes += x;
    d->chain_internal.assign(internal.begin(), internal.end());
}

// Every entry of the dense index tables the specialised kernels read with scalar loads must address a row that exists:
// variable classes {node < N, first edge + degree <= E}, check classes edge < E, chain links node <= N (0 = none).
// Always on (O(E) at creation); an inconsistency here would be an out-of-range row in every launch.
static int validate_fast_index(const lutldpc_decoder *d) {
    const size_t n = d->fast_idx.size();
    int rc = LUTLDPC_OK;
    // the table of cnt entries at off lies inside the blob, and every `step`-th entry from `first` on in [0, hi); the first failure stays
    auto check = [&](const char *name, int off, size_t cnt, size_t first, size_t step, int hi) {
        if (rc) return;
        if (off < 0 || (size_t)off + cnt > n) { rc = fail(LUTLDPC_ERR_STATE, std::string("index table check failed: ") + name + " table outside the blob"); return; }
        for (size_t j = first; j < cnt && !rc; j += step)
            if (d->fast_idx[(size_t)off + j] < 0 || d->fast_idx[(size_t)off + j] >= hi) rc = fail(LUTLDPC_ERR_STATE, std::string("index table check failed: ") + name + " entry out of range");
    };
    for (const auto &c : d->vclass) {
        const size_t m = c.nodes.size(), r = (size_t)c.red_n;
        const int N = d->nvar, e_hi = d->E - c.deg + 1;
        check("variable class", c.idx_off, 2 * m, 0, 2, N); check("variable class", c.idx_off, 2 * m, 1, 2, e_hi);        // {node, first edge} per node
        if (c.red_off >= 0) { check("reduced variable class", c.red_off, 2 * r, 0, 2, N); check("reduced variable class", c.red_off, 2 * r, 1, 2, e_hi); }
        check("transposed variable class", c.tidx_off, m, 0, 1, N); check("transposed variable class", c.tidx_off, 2 * m, m, 1, e_hi);      // m nodes, then m first edges
    }
    for (const auto &c : d->cclass) {
        const size_t cnt = c.nodes.size() * (size_t)c.deg;
        check("check class edge", c.idx_off, cnt, 0, 1, d->E); check("check class node", c.nidx_off, cnt, 0, 1, d->nvar);
        check("transposed check class edge", c.tidx_off, cnt, 0, 1, d->E); check("transposed check class node", c.tnidx_off, cnt, 0, 1, d->nvar);
        if (c.chain_off >= 0) check("chain link", c.chain_off, 2 * c.nodes.size(), 0, 1, d->nvar + 1);
    }
    return rc;
}

// the tables of a compiled form join the blob (full-label tables on a 16-byte boundary)
static void append_tables(lutldpc_decoder *d, ProgramForm &f, bool align16) {
    while (align16 && (d->all_tables.size() & 15)) d->all_tables.push_back(0);
    f.tab = {(int)d->all_tables.size(), (int)f.prog.tables.size()};
    d->all_tables.insert(d->all_tables.end(), f.prog.tables.begin(), f.prog.tables.end());
}

// the packed root rows of a balanced variable tree and the scaled table of its top inner node join the blob (pack_root_rows);
// a tree whose tables do not fit the form keeps rows_off = -1 (fast_covers: nibble rows then take the generated kernel)
static void add_root_rows(lutldpc_decoder *d, FastClassPlan &f, int deg) {
    if (!f.ok || deg < 3) return;
    const int root = f.n_tables - 1, top = root - 1;
    std::vector<uint8_t> rows, top4;
    if (!pack_root_rows(d->all_tables.data() + f.tab_off[root], (size_t)f.tab_len[root], f.tab_shift[root],
                        d->all_tables.data() + f.tab_off[top], (size_t)f.tab_len[top], rows, top4)) return;
    auto append = [&](const std::vector<uint8_t> &t) {
        while (d->all_tables.size() & 3) d->all_tables.push_back(0);
        const int32_t off = (int32_t)d->all_tables.size();
        d->all_tables.insert(d->all_tables.end(), t.begin(), t.end());
        return off;
    };
    f.rows_off = append(rows);
    f.top4_off = append(top4);
    while (d->all_tables.size() & 3) d->all_tables.push_back(0);
}

// Compile the trees of one kind of tree set s -- the trees as they are, with their look-ups (all_ops) and the balanced-tree
// plans -- into the base form of every degree class, then the checks' full-label form of it.
static int add_forms(lutldpc_decoder *d, int kind, int s) {
    const std::vector<Tree> &trees = (kind == TT_CHK ? d->chk_trees : d->var_trees)[(size_t)s];
    const std::vector<NodeClass> &cls = kind == TT_CHK ? d->cclass : d->vclass;
    TreeSetPlan &S = *d->tree_set(kind, s);
    S.cls.assign(cls.size(), TreeClassPlan());
    for (size_t i = 0; i < cls.size(); i++) {
        if (cls[i].tree_class >= (int)trees.size()) return fail(LUTLDPC_ERR_ARG, "tree set is missing a degree class");
        const Tree &t = trees[(size_t)cls[i].tree_class];
        TreeClassPlan &c = S.cls[i];
        ProgramForm &f = c.base;
        std::string e;
        if (!compile_program(t, kind, cls[i].deg, f.prog, e)) return fail(LUTLDPC_ERR_UNSUPPORTED, "degree " + std::to_string(cls[i].deg) + ": " + e);
        append_tables(d, f, false);
        if (interp_slot_bytes(f.prog) > 60 * 1024) return fail(LUTLDPC_ERR_UNSUPPORTED, "node program needs more than 60 KiB of LDS slots");     // (the interpreter's)
        c.op_off = (int)d->all_ops.size();
        d->all_ops.insert(d->all_ops.end(), f.prog.ops.begin(), f.prog.ops.end());
        if (kind != TT_CHK) {
            std::map<const TreeNode *, std::pair<uint32_t, uint32_t>> tab_of;
            for (auto &nt : f.prog.node_tabs) tab_of[nt.first] = {(uint32_t)f.tab.off + nt.second[0], nt.second[1]};
            c.fast = plan_fast_vn(t, kind, cls[i].deg, tab_of);
            if (kind == TT_VAR) add_root_rows(d, c.fast, cls[i].deg);
        }
    }
    S.valid = true;
    for (size_t i = 0; i < cls.size() && kind == TT_CHK && d->opt.chk_full_labels; i++) {
        ProgramForm f;
        if (!chk_full_label_program(S.cls[i].base.prog, f.prog) || f.prog.tables.empty()) continue;
        append_tables(d, f, true);
        S.cls[i].full = std::move(f);
    }
    return LUTLDPC_OK;
}

int compile_all(lutldpc_decoder *d) {
    std::string err;
    build_fast_index(d);
    if (int rc = validate_fast_index(d)) return rc;
    // match trees to degree classes like set_trees (src/LDPC_Code_LUT.cpp:133-139,152-158):
    // VARTREE leaves == dv, CHKTREE leaves + 1 == dc, matched on tree set 0
    if (d->var_trees.empty()) return fail(LUTLDPC_ERR_ARG, "no variable-node trees");
    int n_sets = 0;
    for (int i = 0; i < d->max_iters_created; i++) n_sets = std::max(n_sets, d->iter_set[(size_t)i] + 1);
    if ((int)d->var_trees.size() < n_sets) return fail(LUTLDPC_ERR_ARG, "fewer variable tree sets than reuse_vec requires");
    for (auto &c : d->vclass) {
        c.tree_class = -1;
        for (size_t k = 0; k < d->var_trees[0].size(); k++) if (d->var_trees[0][k].num_leaves == c.deg) { c.tree_class = (int)k; break; }
        if (c.tree_class < 0) return fail(LUTLDPC_ERR_ARG, "no variable tree for degree " + std::to_string(c.deg));
    }
    if (!d->min_lut) {
        if ((int)d->chk_trees.size() < n_sets) return fail(LUTLDPC_ERR_ARG, "fewer check tree sets than reuse_vec requires");
        for (auto &c : d->cclass) {
            c.tree_class = -1;
            for (size_t k = 0; k < d->chk_trees[0].size(); k++) if (d->chk_trees[0][k].num_leaves + 1 == c.deg) { c.tree_class = (int)k; break; }
            if (c.tree_class < 0) return fail(LUTLDPC_ERR_ARG, "no check tree for degree " + std::to_string(c.deg));
        }
    }
    d->all_ops.clear(); d->all_tables.clear();
    for (auto &plans : d->tree_plans) plans.assign((size_t)n_sets, TreeSetPlan());
    for (int s = 0; s < n_sets; s++) {
        // a set is either message-update trees or (the last one) decision trees
        const int vkind = !d->var_trees[(size_t)s].empty() && d->var_trees[(size_t)s][0].type == TT_DEC ? TT_DEC : TT_VAR;
        // the order in which the forms reach the blobs is the layout of the blobs
        int rc;
        if ((rc = add_forms(d, vkind, s))) return rc;
        if (!d->min_lut && (rc = add_forms(d, TT_CHK, s))) return rc;
    }
    return LUTLDPC_OK;
}

// Process-wide registry of the run-time generated kernels, keyed by device + source text.  Decoders share the loaded
// modules (equal tree shapes give equal sources: no second hiprtc run), and a module is NEVER unloaded while the process
// lives: unloading frees executable device memory that the runtime hands to the next code object it loads, and the one
// device fault this library has shown ("The round-1 abort") was the first launch of a lazily loaded code object
// right after the modules of the previous decoder had been unloaded.  Bounded: beyond kJitRegistryMax distinct sources the
// generated kernels are simply not used (the interpreter runs instead).
JitRegistry &jit_registry() { static JitRegistry *r = new JitRegistry; return *r; }     // never destroyed (see above)

// The kernel of `src` on `device`: from the registry, else compiled, loaded and remembered -- a failure too (an entry that is not
// ok(); `log` receives the diagnostic of a failure that happened in this call only).  nullptr: the registry is full.
JitKernel *jit_get(int device, const std::string &src, std::string &log) {
    JitRegistry &reg = jit_registry();
    std::lock_guard<std::mutex> lock(reg.mu);
    const std::string key = std::to_string(device) + "\n" + src;
    auto it = reg.by_src.find(key);
    if (it == reg.by_src.end()) {
        if (reg.by_src.size() >= kJitRegistryMax) return nullptr;
        std::vector<char> code; JitKernel k; std::string out;      // (out: hiprtc may leave warnings on success, not handed on)
        if (!jit_compile(src, code, out) || !jit_load(code, k, out)) { k = JitKernel(); log = out.empty() ? "hiprtc returned no code object" : out; }
        it = reg.by_src.emplace(key, k).first;
    }
    return &it->second;                                   // (std::map nodes are stable: the pointer outlives the lock)
}

// Source of the streaming pass kernel of class i of tree set s as build_jit compiles it.  kind: TT_VAR, TT_DEC, TT_CHK (the
// sign/magnitude program) or TT_CHK + 32 (the full-label program, with its own table blob)
bool jit_class_source(const lutldpc_decoder *d, int kind, size_t s, size_t i, std::string &src, std::string &err) {
    const bool full = kind == TT_CHK + 32;
    const TreeClassPlan *c = d->tree_class(full ? TT_CHK : kind, (int)s, (int)i);
    if (!c || (full && c->full.tab.bytes == 0)) { err = "only variable / decision / check-tree programs are generated"; return false; }
    const ProgramForm &f = full ? c->full : c->base;
    return full || kind == TT_CHK ? jit_cn_source(f.prog, d->cclass[i].deg, d->pack, f.tab.bytes, src, err)
                                 : jit_vn_source(f.prog, kind, d->vclass[i].deg, d->pack, f.tab.bytes, src, err);
}

// HIP loads the code object of a translation unit lazily, at the first launch of one of its kernels -- possibly in the
// middle of a decode and long after other modules came and went.  Load all of them at the first decoder creation on a
// device instead, while nothing of ours is in flight.
static int preload_code_objects(int device) {
    static std::mutex mu;
    static std::vector<int> done;
    std::lock_guard<std::mutex> lock(mu);
    if (std::find(done.begin(), done.end(), device) != done.end()) return LUTLDPC_OK;
    HIP_TRY(preload_stream_kernels()); HIP_TRY(preload_frontend_kernels()); HIP_TRY(preload_encode_kernels());                             // the units that define kernels of their own
    HIP_TRY((preload_fused<2, 0>())); HIP_TRY((preload_fused<2, 1>())); HIP_TRY((preload_fused<2, 2>())); HIP_TRY((preload_fused<2, 3>()));
    HIP_TRY((preload_vn_fast<TT_VAR, 1>())); HIP_TRY((preload_vn_fast<TT_VAR, 2>())); HIP_TRY((preload_vn_fast<TT_DEC, 2>()));
    HIP_TRY((preload_cn_fast<2>()));
    HIP_TRY(preload_compact_kernels());
    HIP_TRY(preload_stats_kernels());
    HIP_TRY(preload_events_kernels());
    HIP_TRY(preload_layout_kernels());
    HIP_TRY(preload_llr_kernels());
    HIP_TRY(hipDeviceSynchronize());
    done.push_back(device);
    return LUTLDPC_OK;
}

// jit.hpp: generate + compile + load a kernel for every variable / decision / CHKTREE class without a compile-time specialised one
static void build_jit(lutldpc_decoder *d) {
    if (!d->opt.use_jit || !d->opt.use_fast) return;
    for (size_t s = 0; s < d->tree_plans[TT_VAR].size(); s++)
        for (int kind : {TT_VAR, TT_DEC, TT_CHK}) {
            TreeSetPlan &S = *d->tree_set(kind, (int)s);
            const auto &cls = kind == TT_CHK ? d->cclass : d->vclass;
            for (size_t i = 0; i < S.cls.size(); i++) {
                if (kind != TT_CHK && fast_covers(d, S.cls[i].fast, kind, cls[i].deg)) continue;
                std::string src, log;
                const bool full = kind == TT_CHK && d->chk_form((int)s, (int)i) == &S.cls[i].full;
                if (!jit_class_source(d, full ? TT_CHK + 32 : kind, s, i, src, log)) { d->jit_log = log; continue; }
                JitKernel *k = jit_get(d->device, src, log);
                if (!k) { d->jit_log = "generated-kernel registry full"; continue; }
                if (!log.empty()) d->jit_log = log;
                if (k->ok()) S.cls[i].jit = k;
            }
        }
}

int upload_static(lutldpc_decoder *d) {
    HIP_TRY(hipSetDevice(d->device));
    if (int rc = preload_code_objects(d->device)) return rc;
    HIP_TRY(hipStreamCreateWithFlags(&d->stream.s, hipStreamNonBlocking));
    HIP_TRY(d->d_vn_ptr.upload(d->vn_ptr));
    HIP_TRY(d->d_cn_ptr.upload(d->cn_ptr));
    {   // syndrome kernel: node of every check-edge, bit 31 = last edge of its check, 8 entries of padding
        std::vector<int32_t> f((size_t)d->E + 8, 0);
        for (int c = 0; c < d->nchk; c++)
            for (int k = d->cn_ptr[(size_t)c]; k < d->cn_ptr[(size_t)c + 1]; k++)
                f[(size_t)k] = (int32_t)((uint32_t)d->cn_vn[(size_t)k] | (k + 1 == d->cn_ptr[(size_t)c + 1] ? 0x80000000u : 0u));
        HIP_TRY(d->d_cn_vn.upload(f));
    }
    HIP_TRY(d->d_fast_idx.upload(d->fast_idx));
    HIP_TRY(d->d_chain_internal.upload(d->chain_internal));
    HIP_TRY(d->d_edge_vn.upload(d->edge_vn));
    HIP_TRY(d->d_ops.upload(d->all_ops));
    {   // pad the table blob so that dword staging never reads past the end
        std::vector<uint8_t> t = d->all_tables;
        t.resize((t.size() + 3) / 4 * 4 + 16, 0);
        HIP_TRY(d->d_tables.upload(t));
    }
    build_jit(d);
    return LUTLDPC_OK;
}

#pragma GCC visibility pop
