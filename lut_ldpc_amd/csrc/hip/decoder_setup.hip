// decoder_setup.hip -- what a decoder is made of at creation: degree classes, compiled tree programs, the dense index tables of
// the specialised kernels (with the chain links), the run-time generated kernels and the static uploads.
#include "decoder_state.hpp"

#pragma GCC visibility push(hidden)

// ----------------------------------------------------------------------------- set-up helpers
void build_classes(const std::vector<int> &deg, std::vector<NodeClass> &cls, std::vector<int> &list) {
    std::map<int, std::vector<int>> by;
    for (size_t i = 0; i < deg.size(); i++) by[deg[i]].push_back((int)i);
    cls.clear(); list.clear();
    for (auto &kv : by) { NodeClass c; c.deg = kv.first; c.nodes = kv.second; cls.push_back(std::move(c)); }
    for (auto &c : cls) list.insert(list.end(), c.nodes.begin(), c.nodes.end());
}

// Build the launch plan of one pass from per-class programs (generic) -- progs may be empty
// for the min-sum pass.
static int build_plan(lutldpc_decoder *d, const std::vector<NodeClass> &cls, const std::vector<Program> *progs,
               const std::vector<size_t> *op_off, const std::vector<size_t> *tab_off, PassPlan &plan) {
    if ((int)cls.size() > kMaxSeg) return fail(LUTLDPC_ERR_UNSUPPORTED, "more than 32 distinct node degrees in one pass");
    PassParams &P = plan.P;
    std::memset(&P, 0, sizeof(P));
    P.n_seg = (int)cls.size();
    P.nodes_per_block = d->opt.nodes_per_block;
    P.E = d->E; P.N = d->nvar;
    int blk = 0, node_off = 0, max_slots = 0, max_tab = 0, max_out = 1;
    for (size_t i = 0; i < cls.size(); i++) {
        PassSeg &S = P.seg[i];
        S.block_begin = blk;
        S.n_nodes = (int)cls[i].nodes.size();
        S.node_off = node_off;
        S.deg = cls[i].deg;
        if (progs) {
            const Program &pr = (*progs)[i];
            S.op_off = (int)(*op_off)[i]; S.n_ops = (int)pr.ops.size();
            S.tab_off = (int)(*tab_off)[i]; S.tab_bytes = (int)pr.tables.size();
            S.n_in = pr.n_in; S.n_out = pr.n_out; S.n_slots = pr.n_slots;
            max_slots = std::max(max_slots, pr.n_slots);
            max_tab = std::max(max_tab, (int)pr.tables.size());
            max_out = std::max(max_out, pr.n_out);
        }
        blk += (S.n_nodes + P.nodes_per_block - 1) / P.nodes_per_block;
        node_off += S.n_nodes;
    }
    P.blocks_per_group = blk;
    P.slots_lds = max_slots;
    plan.out_slots = max_out;
    int slots_bytes = (max_slots + max_out) * kWave * 4;
    if (slots_bytes > 60 * 1024) return fail(LUTLDPC_ERR_UNSUPPORTED, "node program needs more than 60 KiB of LDS slots");
    plan.lds_tab = (slots_bytes + max_tab) <= 64 * 1024;
    plan.lds_bytes = slots_bytes + (plan.lds_tab ? max_tab : 0);
    plan.valid = true;
    return LUTLDPC_OK;
}

static void build_fast_index(lutldpc_decoder *d) {
    d->fast_idx.clear(); d->vn_idx_off.clear(); d->cn_idx_off.clear();
    d->chain_idx_off.assign(d->cclass.size(), -1); d->vn_red_off.assign(d->vclass.size(), -1); d->vn_red_n.assign(d->vclass.size(), 0);
    for (auto &c : d->vclass) {
        d->vn_idx_off.push_back((int)d->fast_idx.size());
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
    d->cn_npw_class.assign(d->cclass.size(), 0);
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
                d->cn_npw_class[ci] = std::max(4, d->npw_cn(d->cclass[ci].deg));
                if (d->opt.cn_edges_per_wave <= 0) d->cn_npw_class[ci] = std::max(d->cn_npw_class[ci], std::min(12, n / 2048));
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
        d->cn_idx_off.push_back((int)d->fast_idx.size());
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
            d->chain_idx_off[ci] = (int)d->fast_idx.size();
            for (int cn : c.nodes) { d->fast_idx.push_back(back[(size_t)cn]); d->fast_idx.push_back(fwd[(size_t)cn]); }
        }
    }
    // the node behind every entry of the check classes' edge tables, same order
    {
        std::vector<int> edge_node((size_t)d->E, 0);
        for (int v = 0; v < d->nvar; v++)
            for (int e = d->vn_ptr[(size_t)v]; e < d->vn_ptr[(size_t)v + 1]; e++) edge_node[(size_t)e] = v;
        d->cn_nidx_off.assign(d->cclass.size(), 0);
        for (size_t ci = 0; ci < d->cclass.size(); ci++) {
            const size_t off = (size_t)d->cn_idx_off[ci], cnt = d->cclass[ci].nodes.size() * (size_t)d->cclass[ci].deg;
            d->cn_nidx_off[ci] = (int)d->fast_idx.size();
            for (size_t j = 0; j < cnt; j++) d->fast_idx.push_back(edge_node[(size_t)d->fast_idx[off + j]]);
        }
    }
    // LDS-resident decoder (jit_resident.hpp): there a LANE owns a node, so the tables are transposed -- [k][node of the class] --
    // and 64 lanes reading entry k of 64 consecutive nodes touch 256 contiguous bytes.  Canonical edge order of the check
    // (ascending variable node, as cn_msg_idx: a CHKTREE consumes its inputs in that order).
    {
        std::vector<int> edge_node((size_t)d->E, 0);
        for (int v = 0; v < d->nvar; v++)
            for (int e = d->vn_ptr[(size_t)v]; e < d->vn_ptr[(size_t)v + 1]; e++) edge_node[(size_t)e] = v;
        d->cn_tidx_off.assign(d->cclass.size(), 0); d->cn_tnidx_off.assign(d->cclass.size(), 0); d->vn_tidx_off.assign(d->vclass.size(), 0);
        for (size_t ci = 0; ci < d->cclass.size(); ci++) {
            const auto &c = d->cclass[ci];
            const size_t n = c.nodes.size();
            d->cn_tidx_off[ci] = (int)d->fast_idx.size();
            for (int k = 0; k < c.deg; k++) for (size_t j = 0; j < n; j++) d->fast_idx.push_back(d->cn_msg_idx[(size_t)(d->cn_ptr[(size_t)c.nodes[j]] + k)]);
            d->cn_tnidx_off[ci] = (int)d->fast_idx.size();
            for (int k = 0; k < c.deg; k++) for (size_t j = 0; j < n; j++) d->fast_idx.push_back(edge_node[(size_t)d->cn_msg_idx[(size_t)(d->cn_ptr[(size_t)c.nodes[j]] + k)]]);
        }
        for (size_t vi = 0; vi < d->vclass.size(); vi++) {
            const auto &c = d->vclass[vi];
            d->vn_tidx_off[vi] = (int)d->fast_idx.size();
            for (int v : c.nodes) d->fast_idx.push_back(v);
            for (int v : c.nodes) d->fast_idx.push_back(d->vn_ptr[(size_t)v]);
        }
    }
    // variable passes that follow a chained check pass skip the nodes it already updated
    for (size_t vi = 0; vi < d->vclass.size(); vi++) {
        if (d->vclass[vi].deg != 2) continue;
        d->vn_red_off[vi] = (int)d->fast_idx.size();
        for (int v : d->vclass[vi].nodes)
            if (!internal[(size_t)v]) { d->fast_idx.push_back(v); d->fast_idx.push_back(d->vn_ptr[(size_t)v]); d->vn_red_n[vi]++; }
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
    auto bad = [&](const std::string &what) { return fail(LUTLDPC_ERR_STATE, "index table check failed: " + what); };
    for (size_t i = 0; i < d->vclass.size(); i++) {
        const auto &c = d->vclass[i];
        const size_t off = (size_t)d->vn_idx_off[i];
        if (off + 2 * c.nodes.size() > n) return bad("variable class table outside the blob");
        for (size_t j = 0; j < c.nodes.size(); j++) {
            const int v = d->fast_idx[off + 2 * j], e = d->fast_idx[off + 2 * j + 1];
            if (v < 0 || v >= d->nvar || e < 0 || e + c.deg > d->E) return bad("variable node / first edge out of range");
        }
        if (d->vn_red_off[i] >= 0) {
            const size_t ro = (size_t)d->vn_red_off[i];
            if (ro + 2 * (size_t)d->vn_red_n[i] > n) return bad("reduced variable class table outside the blob");
            for (int j = 0; j < d->vn_red_n[i]; j++) {
                const int v = d->fast_idx[ro + 2 * (size_t)j], e = d->fast_idx[ro + 2 * (size_t)j + 1];
                if (v < 0 || v >= d->nvar || e < 0 || e + c.deg > d->E) return bad("reduced variable class entry out of range");
            }
        }
    }
    for (size_t i = 0; i < d->vclass.size() && i < d->vn_tidx_off.size(); i++) {
        const auto &c = d->vclass[i];
        const size_t off = (size_t)d->vn_tidx_off[i], m = c.nodes.size();
        if (off + 2 * m > n) return bad("transposed variable class table outside the blob");
        for (size_t j = 0; j < m; j++) {
            const int v = d->fast_idx[off + j], e = d->fast_idx[off + m + j];
            if (v < 0 || v >= d->nvar || e < 0 || e + c.deg > d->E) return bad("transposed variable class entry out of range");
        }
    }
    for (size_t i = 0; i < d->cclass.size() && i < d->cn_tidx_off.size(); i++) {
        const auto &c = d->cclass[i];
        const size_t cnt = c.nodes.size() * (size_t)c.deg, eo = (size_t)d->cn_tidx_off[i], no = (size_t)d->cn_tnidx_off[i];
        if (eo + cnt > n || no + cnt > n) return bad("transposed check class table outside the blob");
        for (size_t j = 0; j < cnt; j++) if (d->fast_idx[eo + j] < 0 || d->fast_idx[eo + j] >= d->E || d->fast_idx[no + j] < 0 || d->fast_idx[no + j] >= d->nvar) return bad("transposed check class entry out of range");
    }
    for (size_t i = 0; i < d->cclass.size(); i++) {
        const auto &c = d->cclass[i];
        const size_t off = (size_t)d->cn_idx_off[i], cnt = c.nodes.size() * (size_t)c.deg;
        if (off + cnt > n) return bad("check class table outside the blob");
        for (size_t j = 0; j < cnt; j++) if (d->fast_idx[off + j] < 0 || d->fast_idx[off + j] >= d->E) return bad("check edge out of range");
        if (i < d->cn_nidx_off.size()) {
            const size_t no = (size_t)d->cn_nidx_off[i];
            if (no + cnt > n) return bad("check class node table outside the blob");
            for (size_t j = 0; j < cnt; j++) if (d->fast_idx[no + j] < 0 || d->fast_idx[no + j] >= d->nvar) return bad("check node out of range");
        }
        if (d->chain_idx_off[i] >= 0) {
            const size_t co = (size_t)d->chain_idx_off[i];
            if (co + 2 * c.nodes.size() > n) return bad("chain link table outside the blob");
            for (size_t j = 0; j < 2 * c.nodes.size(); j++) if (d->fast_idx[co + j] < 0 || d->fast_idx[co + j] > d->nvar) return bad("chain link out of range");
        }
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
    auto add_set = [&](const std::vector<Tree> &trees, const std::vector<NodeClass> &cls, int kind,
                       std::vector<Program> &progs, PassPlan &plan, std::vector<FastClassPlan> *fast) -> int {
        progs.resize(cls.size());
        if (fast) fast->assign(cls.size(), FastClassPlan());
        std::vector<size_t> op_off(cls.size()), tab_off(cls.size());
        for (size_t i = 0; i < cls.size(); i++) {
            if (cls[i].tree_class >= (int)trees.size()) return fail(LUTLDPC_ERR_ARG, "tree set is missing a degree class");
            const Tree &t = trees[(size_t)cls[i].tree_class];
            std::string e;
            if (!compile_program(t, kind, cls[i].deg, progs[i], e))
                return fail(LUTLDPC_ERR_UNSUPPORTED, "degree " + std::to_string(cls[i].deg) + ": " + e);
            op_off[i] = d->all_ops.size(); tab_off[i] = d->all_tables.size();
            d->all_ops.insert(d->all_ops.end(), progs[i].ops.begin(), progs[i].ops.end());
            d->all_tables.insert(d->all_tables.end(), progs[i].tables.begin(), progs[i].tables.end());
            if (fast) {
                std::map<const TreeNode *, std::pair<uint32_t, uint32_t>> tab_of;
                for (auto &nt : progs[i].node_tabs) tab_of[nt.first] = {(uint32_t)tab_off[i] + nt.second[0], nt.second[1]};
                (*fast)[i] = plan_fast_vn(t, kind, cls[i].deg, tab_of);
            }
        }
        return build_plan(d, cls, &progs, &op_off, &tab_off, plan);
    };
    // composed variants of the programs of one set (tables appended to the same blob).  Off by default (LUTLDPC_COMPOSE=1), measured
    // on MI355X (tools/resident_probe.py): a 4 KB table spreads its 1024 dwords over 32 banks 32 deep -- the three-input look-ups run
    // into 3-4-way bank conflicts where a 256-byte table has at most two dwords per bank -- and the halved look-up count does not pay
    // for it: (3,6) N=10000 1.72 -> 1.24 M codewords/s with composition.
    auto add_composed = [&](const std::vector<Tree> &trees, const std::vector<NodeClass> &cls, int kind, std::vector<Program> &progs,
                            std::vector<std::pair<int, int>> &tabs) -> int {
        progs.assign(cls.size(), Program()); tabs.assign(cls.size(), {0, 0});
        for (size_t i = 0; i < cls.size(); i++) {
            const Tree &t = trees[(size_t)cls[i].tree_class];
            const Tree tc = d->opt.use_compose ? compose_tree(t, kind, (uint64_t)d->opt.compose_space) : compose_tree(t, kind, 0);
            std::string e;
            if (!compile_program(tc, kind, cls[i].deg, progs[i], e)) return fail(LUTLDPC_ERR_UNSUPPORTED, "composed tree, degree " + std::to_string(cls[i].deg) + ": " + e);
            progs[i].node_tabs.clear();                         // (they point into the temporary tree)
            tabs[i] = {(int)d->all_tables.size(), (int)progs[i].tables.size()};
            d->all_tables.insert(d->all_tables.end(), progs[i].tables.begin(), progs[i].tables.end());
        }
        return LUTLDPC_OK;
    };
    size_t ns = (size_t)n_sets;
    d->var_prog.assign(ns, {}); d->dec_prog.assign(ns, {}); d->chk_prog.assign(ns, {});
    d->var_plan.assign(ns, {}); d->dec_plan.assign(ns, {}); d->chk_plan.assign(ns, {});
    d->var_fast.assign(ns, {}); d->dec_fast.assign(ns, {});
    d->chk_prog_full.assign(ns, {}); d->chk_full_tab.assign(ns, {});
    d->chk_prog_cf.assign(ns, {}); d->chk_tab_cf.assign(ns, {});
    d->var_prog_c.assign(ns, {}); d->dec_prog_c.assign(ns, {}); d->chk_prog_c.assign(ns, {});
    d->var_tab_c.assign(ns, {}); d->dec_tab_c.assign(ns, {}); d->chk_tab_c.assign(ns, {});
    for (size_t s = 0; s < ns; s++) {
        // a set is either message-update trees or (the last one) decision trees
        int type = d->var_trees[s].empty() ? TT_VAR : d->var_trees[s][0].type;
        int rc;
        if (type == TT_DEC) rc = add_set(d->var_trees[s], d->vclass, TT_DEC, d->dec_prog[s], d->dec_plan[s], &d->dec_fast[s]);
        else rc = add_set(d->var_trees[s], d->vclass, TT_VAR, d->var_prog[s], d->var_plan[s], &d->var_fast[s]);
        if (rc) return rc;
        if (!d->min_lut) {
            rc = add_set(d->chk_trees[s], d->cclass, TT_CHK, d->chk_prog[s], d->chk_plan[s], nullptr);
            if (rc) return rc;
            d->chk_prog_full[s].assign(d->cclass.size(), Program());
            d->chk_full_tab[s].assign(d->cclass.size(), {0, 0});
            for (size_t i = 0; i < d->cclass.size() && d->opt.chk_full_labels; i++) {
                Program f;
                if (!chk_full_label_program(d->chk_prog[s][i], f) || f.tables.empty()) continue;
                while (d->all_tables.size() & 15) d->all_tables.push_back(0);
                d->chk_full_tab[s][i] = {(int)d->all_tables.size(), (int)f.tables.size()};
                d->all_tables.insert(d->all_tables.end(), f.tables.begin(), f.tables.end());
                d->chk_prog_full[s][i] = std::move(f);
            }
        }
        if (type == TT_DEC) rc = add_composed(d->var_trees[s], d->vclass, TT_DEC, d->dec_prog_c[s], d->dec_tab_c[s]);
        else rc = add_composed(d->var_trees[s], d->vclass, TT_VAR, d->var_prog_c[s], d->var_tab_c[s]);
        if (rc) return rc;
        if (!d->min_lut && (rc = add_composed(d->chk_trees[s], d->cclass, TT_CHK, d->chk_prog_c[s], d->chk_tab_c[s]))) return rc;
        if (!d->min_lut) {
            d->chk_prog_cf[s].assign(d->cclass.size(), Program());
            d->chk_tab_cf[s].assign(d->cclass.size(), {0, 0});
            for (size_t i = 0; i < d->cclass.size() && d->opt.chk_full_labels; i++) {
                Program f;
                if (!chk_full_label_program(d->chk_prog_c[s][i], f) || f.tables.empty()) continue;
                while (d->all_tables.size() & 15) d->all_tables.push_back(0);
                d->chk_tab_cf[s][i] = {(int)d->all_tables.size(), (int)f.tables.size()};
                d->all_tables.insert(d->all_tables.end(), f.tables.begin(), f.tables.end());
                d->chk_prog_cf[s][i] = std::move(f);
            }
        }
    }
    if (d->min_lut) { int rc = build_plan(d, d->cclass, nullptr, nullptr, nullptr, d->cn_minsum_plan); if (rc) return rc; }
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
    if (kind == TT_CHK + 32 && s < d->chk_full_tab.size() && i < d->chk_full_tab[s].size() && d->chk_full_tab[s][i].second > 0)
        return jit_cn_source(d->chk_prog_full[s][i], d->cclass[i].deg, d->pack, d->chk_full_tab[s][i].second, src, err);
    if (kind != TT_VAR && kind != TT_DEC && kind != TT_CHK) { err = "only variable / decision / check-tree programs are generated"; return false; }
    const PassPlan &plan = kind == TT_VAR ? d->var_plan[s] : kind == TT_DEC ? d->dec_plan[s] : d->chk_plan[s];
    const auto &progs = kind == TT_VAR ? d->var_prog[s] : kind == TT_DEC ? d->dec_prog[s] : d->chk_prog[s];
    return kind == TT_CHK ? jit_cn_source(progs[i], d->cclass[i].deg, d->pack, plan.P.seg[i].tab_bytes, src, err)
                          : jit_vn_source(progs[i], kind, d->vclass[i].deg, d->pack, plan.P.seg[i].tab_bytes, src, err);
}

// HIP loads the code object of a translation unit lazily, at the first launch of one of its kernels -- possibly in the
// middle of a decode and long after other modules came and went.  Load all of them at the first decoder creation on a
// device instead, while nothing of ours is in flight.
static int preload_code_objects(int device) {
    static std::mutex mu;
    static std::vector<int> done;
    std::lock_guard<std::mutex> lock(mu);
    if (std::find(done.begin(), done.end(), device) != done.end()) return LUTLDPC_OK;
    HIP_TRY(preload_stream_kernels()); HIP_TRY(preload_frontend_kernels());                             // the units that define kernels of their own
    HIP_TRY((preload_fused<2, 0>())); HIP_TRY((preload_fused<2, 1>())); HIP_TRY((preload_fused<2, 2>())); HIP_TRY((preload_fused<2, 3>()));
    HIP_TRY((preload_vn_fast<TT_VAR, 1>())); HIP_TRY((preload_vn_fast<TT_VAR, 2>())); HIP_TRY((preload_vn_fast<TT_DEC, 2>()));
    HIP_TRY((preload_cn_fast<2>()));
    HIP_TRY(preload_compact_kernels());
    HIP_TRY(preload_stats_kernels());
    HIP_TRY(preload_events_kernels());
    HIP_TRY(hipDeviceSynchronize());
    done.push_back(device);
    return LUTLDPC_OK;
}

// jit.hpp: generate + compile + load a kernel for every variable / decision / CHKTREE class without a compile-time specialised one
static void build_jit(lutldpc_decoder *d) {
    const size_t ns = d->var_plan.size();
    d->var_jit.assign(ns, {}); d->dec_jit.assign(ns, {}); d->chk_jit.assign(ns, {});
    if (!d->opt.use_jit || !d->opt.use_fast) return;
    for (size_t s = 0; s < ns; s++)
        for (int kind : {TT_VAR, TT_DEC, TT_CHK}) {
            if (kind == TT_CHK && d->min_lut) continue;
            const PassPlan &plan = kind == TT_VAR ? d->var_plan[s] : kind == TT_DEC ? d->dec_plan[s] : d->chk_plan[s];
            if (!plan.valid) continue;
            const auto &cls = kind == TT_CHK ? d->cclass : d->vclass;
            auto &out = kind == TT_VAR ? d->var_jit[s] : kind == TT_DEC ? d->dec_jit[s] : d->chk_jit[s];
            out.assign(cls.size(), nullptr);
            for (size_t i = 0; i < cls.size(); i++) {
                if (kind != TT_CHK && fast_covers(d, (kind == TT_VAR ? d->var_fast[s] : d->dec_fast[s])[i], cls[i].deg)) continue;
                std::string src, log;
                const bool full = kind == TT_CHK && s < d->chk_full_tab.size() && i < d->chk_full_tab[s].size() && d->chk_full_tab[s][i].second > 0;
                if (!jit_class_source(d, full ? TT_CHK + 32 : kind, s, i, src, log)) { d->jit_log = log; continue; }
                JitKernel *k = jit_get(d->device, src, log);
                if (!k) { d->jit_log = "generated-kernel registry full"; continue; }
                if (!log.empty()) d->jit_log = log;
                if (k->ok()) out[i] = k;
            }
        }
}

int upload_static(lutldpc_decoder *d) {
    HIP_TRY(hipSetDevice(d->device));
    if (int rc = preload_code_objects(d->device)) return rc;
    HIP_TRY(hipStreamCreateWithFlags(&d->stream.s, hipStreamNonBlocking));
    HIP_TRY(d->d_vn_ptr.upload(d->vn_ptr));
    HIP_TRY(d->d_cn_ptr.upload(d->cn_ptr));
    HIP_TRY(d->d_cn_idx.upload(d->cn_msg_idx));
    {   // syndrome kernel: node of every check-edge, bit 31 = last edge of its check, 8 entries of padding
        std::vector<int32_t> f((size_t)d->E + 8, 0);
        for (int c = 0; c < d->nchk; c++)
            for (int k = d->cn_ptr[(size_t)c]; k < d->cn_ptr[(size_t)c + 1]; k++)
                f[(size_t)k] = (int32_t)((uint32_t)d->cn_vn[(size_t)k] | (k + 1 == d->cn_ptr[(size_t)c + 1] ? 0x80000000u : 0u));
        HIP_TRY(d->d_cn_vn.upload(f));
    }
    HIP_TRY(d->d_vn_list.upload(d->vn_list));
    HIP_TRY(d->d_cn_list.upload(d->cn_list));
    HIP_TRY(d->d_fast_idx.upload(d->fast_idx));
    HIP_TRY(d->d_chain_internal.upload(d->chain_internal));
    d->edge_vn.resize((size_t)d->E);
    for (int v = 0; v < d->nvar; v++) for (int e = d->vn_ptr[(size_t)v]; e < d->vn_ptr[(size_t)v + 1]; e++) d->edge_vn[(size_t)e] = v;
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
