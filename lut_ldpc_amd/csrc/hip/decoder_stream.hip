// decoder_stream.hip -- the streaming decode: one launch per pass and degree class (launch_pass), exit tests, decision pass, message trace,
// graph replay.  Replaces LDPC_Code_LUT::lut_decode and everything below it (src/LDPC_Code_LUT.cpp:259-469,
// src/LUT_Tree.cpp:402-445,774-820) for a BATCH of frames: the frame loop of LDPC_BER_Sim::sim_snr_point
// (src/LDPC_BER_Sim.cpp:260-291) becomes the innermost, coalesced memory dimension.  See kernels_common.hpp for the HBM layout.
// Home of every kernel of kernels_generic.hpp.
#include "decoder_state.hpp"
#include "kernels_generic.hpp"

#pragma GCC visibility push(hidden)

// (see preload_code_objects) this unit's code object
hipError_t preload_stream_kernels() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&frame_state_kernel));
}

int launch_state(lutldpc_decoder *d, int B, int Bpad, int mode, int value, int f0, int f1, int sel) {
    Timed t(d, LUTLDPC_K_LAYOUT);
    if (f1 < 0) f1 = Bpad;
    if (f1 <= f0) return LUTLDPC_OK;
    if (mode == 0) HIP_TRY(hipMemsetAsync(d->d_vfail.p + (size_t)kVfailSlots * d->Bcap, 0, (size_t)kVfailSlots * d->Bcap, d->stream));
    launch_k(frame_state_kernel, dim3((unsigned)((f1 - f0) / 256)), dim3(256), 0, d->stream,
                       d->d_state.p, d->d_vfail.p + (size_t)sel * kVfailSlots * d->Bcap, d->d_iters.p, B, f0, f1, mode, value, d->Bcap);
    LAUNCH_CHECK();
    return LUTLDPC_OK;
}

static int launch_syndrome(lutldpc_decoder *d, int G, int sel = 0) {
    Timed t(d, LUTLDPC_K_SYNDROME);
    const int cpw = 8;
    unsigned bx = (unsigned)((d->nchk + 4 * cpw - 1) / (4 * cpw));
    PACK_DISPATCH(d, launch_k(syndrome_bits_kernel<PK>, dim3(bx, (unsigned)G), dim3(256), 0, d->stream, d->d_hard.p,
                       reinterpret_cast<const uint32_t *>(d->d_state.p), reinterpret_cast<uint32_t *>(d->d_vfail.p + (size_t)sel * kVfailSlots * d->Bcap),
                       d->d_cn_ptr.p, reinterpret_cast<const uint32_t *>(d->d_cn_vn.p), d->nchk, d->nvar, cpw, d->Bcap / 4, -1, (const int32_t *)nullptr, (int32_t *)nullptr));
    LAUNCH_CHECK();
    return LUTLDPC_OK;
}
// The test on the channel decisions (src/LDPC_Code_LUT.cpp:275-279) straight off the channel-label rows: a one-wave probe over
// the first 64 checks of every group, then the full pass, which skips the groups whose frames have all failed in the probe.
// The decided bits of the frames that pass are written at the end of the decode (hard_from_labels_masked_kernel).
static int launch_syndrome_of_labels(lutldpc_decoder *d, int G) {
    Timed t(d, LUTLDPC_K_SYNDROME);
    const int cpw = 8, sbit = __builtin_ctz((unsigned)(d->Nq_Cha / 2));
    HIP_TRY(hipMemsetAsync(d->d_grp.p, 0, sizeof(int32_t) * (size_t)G, d->stream));
#define SYN_ARGS(CPW, SKIP, OUT) d->d_cha_t.p, reinterpret_cast<const uint32_t *>(d->d_state.p), reinterpret_cast<uint32_t *>(d->d_vfail.p), d->d_cn_ptr.p, \
                     reinterpret_cast<const uint32_t *>(d->d_cn_vn.p), d->nchk, d->nvar, CPW, d->Bcap / 4, sbit, SKIP, OUT
    PACK_DISPATCH(d, launch_k(syndrome_bits_kernel<PK>, dim3(1u, (unsigned)G), dim3(64), 0, d->stream, SYN_ARGS(64, (const int32_t *)nullptr, d->d_grp.p)));
    unsigned bx = (unsigned)((d->nchk + 4 * cpw - 1) / (4 * cpw));
    PACK_DISPATCH(d, launch_k(syndrome_bits_kernel<PK>, dim3(bx, (unsigned)G), dim3(256), 0, d->stream, SYN_ARGS(cpw, (const int32_t *)d->d_grp.p, (int32_t *)nullptr)));
#undef SYN_ARGS
    LAUNCH_CHECK();
    return LUTLDPC_OK;
}

// ----------------------------------------------------------------------------- the kernel of a class
PassKernel pass_kernel(const lutldpc_decoder *d, int kind, int set, int cls, int nz) {
    // min-sum checks: the compile-time kernel where it has the shape, else the any-degree, any-alphabet one
    if (kind == TT_CHK && d->min_lut) return d->opt.use_fast && cn_minsum_shape(nz, d->cclass[(size_t)cls].deg) ? KERNEL_FAST : KERNEL_INTERPRETER;
    const TreeClassPlan *t = d->tree_class(kind, set, cls);
    // The compile-time and generated variable kernels read the sign of an outgoing label as bit sbit = log2(nz) (exit test and
    // decided bits); that holds only where nz is a power of two.  A variable pass that writes any other alphabet (Nq_Msg = 12:
    // nz = 6) runs in the interpreter, which compares the label with nz.
    if (!t || (kind == TT_VAR && !is_pow2(nz))) return KERNEL_INTERPRETER;
    if (kind != TT_CHK && fast_covers(d, t->fast, kind, d->vclass[(size_t)cls].deg)) return KERNEL_FAST;
    return t->jit ? KERNEL_GENERATED : KERNEL_INTERPRETER;      // (build_jit: a kernel for every class without a compile-time one)
}

// ----------------------------------------------------------------------------- class parameters
// The only code that fills a ClassParams.  skew_ii = kPerClassLaunch: a launch of the streaming decode (flag buffer 0, no chain,
// inputs from the edge rows) through the kernel pass_kernel names -- an interpreter block takes opt.nodes_per_block nodes, and the
// tables are those of that kernel; otherwise: a role of the skewed pipeline in that iteration (decoder_skew.hip: compile-time kernels).
static ClassParams class_params(const lutldpc_decoder *d, int kind, const NodeClass &c, int n_nodes, int idx_off, int npw, HalfRange g, int nz, int check) {
    ClassParams P{};
    P.kind = kind; P.deg = c.deg; P.g0 = g.g0; P.G = g.G;
    P.n_nodes = n_nodes; P.nodes_per_wave = npw; P.waves_per_group = (n_nodes + npw - 1) / npw;
    P.idx_off = idx_off; P.E = d->E; P.N = d->nvar; P.nz = nz; P.check = check; P.vfail_stride_w = d->Bcap / 4;
    return P;
}
ClassParams cn_class_params(const lutldpc_decoder *d, size_t ci, HalfRange groups, int nz, int check, int skew_ii) {
    const NodeClass &c = d->cclass[ci];
    const int npw = skew_ii != kPerClassLaunch ? d->npw_cn_class(ci) : pass_kernel(d, TT_CHK, 0, (int)ci, nz) == KERNEL_INTERPRETER ? d->opt.nodes_per_block : d->npw_cn(c.deg);
    ClassParams P = class_params(d, 0, c, (int)c.nodes.size(), c.idx_off, npw, groups, nz, check);
    if (skew_ii == kPerClassLaunch) return P;
    const int ii = skew_ii, buf_w = kVfailSlots * d->Bcap / 4;        // words per flag buffer
    P.vfail_off_w = (ii & 1) * buf_w;                                 // parity flags: this iteration's exit test
    if (ii == 0 && d->opt.first_from_nodes) { P.first = 1; P.nidx_off = c.nidx_off; }
    const bool on = ii != d->max_iters - 1 && chain_active(d, d->iter_set[(size_t)ii]);
    // decided bits of the nodes updated here: stored by the check pass that reads their messages, unless they are recovered at
    // the end with everything else (late_hard_active + chain_hard_kernel)
    const bool hard = d->psc && ii >= 1 && chain_active(d, d->iter_set[(size_t)(ii - 1)]) && !late_hard_active(d, true, nullptr);
    if ((on || hard) && c.chain_off >= 0) {
        P.chain.idx_off = c.chain_off;
        P.chain.hard = hard ? 1 : 0;
        if (on) {
            const FastClassPlan &F2 = d->tree_class(TT_VAR, d->iter_set[(size_t)ii], d->chain_vclass)->fast;
            P.chain.on = 1;
            P.chain.tab_off = F2.tab_off[0]; P.chain.tab_len = F2.tab_len[0]; P.chain.tab_shift = F2.tab_shift[0];
            P.chain.check = d->psc ? 1 : 0;
            P.chain.vfail_off_w = ((ii + 1) & 1) * buf_w;             // unanimity of the nodes updated here: the next exit test
            P.chain.sbit_out = __builtin_ctz((unsigned)(d->Nq_Msg[(size_t)(ii + 1)] / 2) | 0x100u);
        }
    }
    return P;
}
ClassParams lut_cn_class_params(const lutldpc_decoder *d, int set, size_t ci, HalfRange groups, int nz, int check) {
    const NodeClass &c = d->cclass[ci];
    const bool interp = pass_kernel(d, TT_CHK, set, (int)ci, nz) == KERNEL_INTERPRETER;
    ClassParams P = class_params(d, 0, c, (int)c.nodes.size(), c.idx_off, interp ? d->opt.nodes_per_block : d->npw_cn(c.deg), groups, nz, check);
    // the class blob: of the form the kernel was generated for, or the tree as the reference walks it
    const TabRef tab = interp ? d->tree_class(TT_CHK, set, (int)ci)->base.tab : d->chk_form(set, (int)ci)->tab;
    P.tab_off[0] = tab.off; P.tab_len[0] = tab.bytes;
    return P;
}
ClassParams vn_class_params(const lutldpc_decoder *d, int kind, int set, size_t ci, HalfRange groups, int nz, int check, int write_hard, int skew_ii) {
    const NodeClass &c = d->vclass[ci];
    int n_nodes = (int)c.nodes.size(), idx_off = c.idx_off;
    if (skew_ii != kPerClassLaunch && chain_active(d, set) && (int)ci == d->chain_vclass) { n_nodes = c.red_n; idx_off = c.red_off; }   // the others are updated by the check pass
    const PassKernel k = pass_kernel(d, kind, set, (int)ci, nz);
    ClassParams P = class_params(d, 1, c, n_nodes, idx_off, k == KERNEL_INTERPRETER ? d->opt.nodes_per_block : d->npw_vn(c.deg), groups, nz, check);
    P.write_hard = write_hard;
    if (skew_ii != kPerClassLaunch) P.vfail_off_w = ((skew_ii + 1) & 1) * (kVfailSlots * d->Bcap / 4);      // unanimity flags: the exit test after the NEXT check pass
    const TreeClassPlan &t = *d->tree_class(kind, set, (int)ci);
    const FastClassPlan &f = t.fast;
    if (k == KERNEL_FAST) {                                           // balanced tree: its tables in canonical order
        P.shift_msg = f.shift_msg;
        for (int t = 0; t < f.n_tables; t++) { P.tab_off[t] = f.tab_off[t]; P.tab_len[t] = f.tab_len[t]; P.tab_shift[t] = f.tab_shift[t]; }
        if (vn_root_rows(kind, d->pack, c.deg)) {                     // the root as packed rows, the top inner node's table times 4 (fast_covers: the plan has them)
            P.root_rows = 1;
            P.tab_off[f.n_tables - 1] = f.rows_off; P.tab_len[f.n_tables - 1] = kRootRowsBytes;
            P.tab_off[f.n_tables - 2] = f.top4_off;
        }
    } else {                                                          // generated kernel, interpreter: the class blob
        P.tab_off[0] = t.base.tab.off; P.tab_len[0] = t.base.tab.bytes;
    }
    return P;
}

// One ClassParams against the sizes of everything it addresses and the cases of its kernel (LUTLDPC_VALIDATE=1: before every
// per-class launch; always: every role of a skew plan)
int validate_class(const lutldpc_decoder *d, const ClassParams &R, const std::string &where, const KernelCases &k) {
    auto bad = [&](const std::string &what) { return fail(LUTLDPC_ERR_STATE, where + ": " + what); };
    const int groups = d->Bcap / d->tile();
    const size_t idx_n = d->fast_idx.size(), tab_n = d->d_tables.n, vfail_w = d->d_vfail.n / 4;
    auto table_ok = [&](int off, int len, int min_len, int max_len) { return off >= 0 && len >= min_len && len <= max_len && !(off & 3) && (size_t)off + (size_t)len <= tab_n; };
    if (R.G < 1 || R.g0 < 0 || R.g0 + R.G > groups) return bad("frame groups outside the batch buffers");
    if (R.E != d->E || R.N != d->nvar) return bad("E / N");
    if (R.n_nodes < 1 || R.nodes_per_wave < 1 || R.waves_per_group != (R.n_nodes + R.nodes_per_wave - 1) / R.nodes_per_wave) return bad("waves per group");
    if (R.vfail_stride_w != d->Bcap / 4 || R.vfail_off_w < 0 || (size_t)R.vfail_off_w + (size_t)kVfailSlots * (size_t)R.vfail_stride_w > vfail_w) return bad("flag buffer");
    if (R.kind != (k.tree_kind == TT_CHK ? 0 : 1)) return bad("kind");
    if (R.kind == 0) {
        if (R.deg < 2 || R.deg > k.max_cn_deg) return bad(std::string("check degree outside ") + k.limit);
        if (R.idx_off < 0 || (size_t)R.idx_off + (size_t)R.n_nodes * (size_t)R.deg > idx_n) return bad("edge table");
        if (!k.generated && (!is_pow2(R.nz) || R.nz > 64)) return bad("nz");
        if (R.first && (R.nidx_off < 0 || (size_t)R.nidx_off + (size_t)R.n_nodes * (size_t)R.deg > idx_n || R.check || R.chain.hard)) return bad("node table of the first check pass");
        if (R.chain.on || R.chain.hard) {
            if (R.chain.idx_off < 0 || (size_t)R.chain.idx_off + 2 * (size_t)R.n_nodes > idx_n) return bad("chain link table");
            if (R.chain.on && (R.chain.tab_off < 0 || R.chain.tab_len < 4 || R.chain.tab_len > 1024 || (size_t)R.chain.tab_off + (size_t)R.chain.tab_len > tab_n)) return bad("chain table");
            if (R.chain.on && R.chain.check && (R.chain.vfail_off_w < 0 || (size_t)R.chain.vfail_off_w + (size_t)kVfailSlots * (size_t)R.vfail_stride_w > vfail_w)) return bad("chain flag buffer");
        }
    } else {
        if (R.deg < 1 || R.deg > k.max_vn_deg) return bad(std::string("variable degree outside ") + k.limit);
        if (R.idx_off < 0 || (size_t)R.idx_off + 2 * (size_t)R.n_nodes > idx_n) return bad("node table");
    }
    if (k.generated) {
        if (!table_ok(R.tab_off[0], R.tab_len[0], 0, INT32_MAX)) return bad("class tables");
    } else if (R.kind) {
        const int leaves = k.tree_kind == TT_DEC ? R.deg : R.deg - 1, nt = leaves > 1 ? leaves : 1;       // LUT nodes of the balanced tree, root included
        for (int t = 0; t < nt; t++)
            if (!table_ok(R.tab_off[t], R.tab_len[t], 1, kFastTableStride)) return bad("table " + std::to_string(t));
        // the kernel of this (kind, rows, degree) reads the root as packed rows or as bytes: the parameters must say the same
        if ((R.root_rows != 0) != vn_root_rows(k.tree_kind, d->pack, R.deg)) return bad("root rows");
        if (R.root_rows && R.tab_len[nt - 1] != kRootRowsBytes) return bad("packed root rows");
    }
    return LUTLDPC_OK;
}
// LUTLDPC_VALIDATE=1: the parameters of a per-class launch against the allocations, before it is issued
static int check_class_launch(const lutldpc_decoder *d, const ClassParams &P, size_t i, int tree_kind, PassKernel kernel) {
    if (!d->opt.validate) return LUTLDPC_OK;
    const KernelCases k = kernel == KERNEL_FAST        ? KernelCases{tree_kind, false, kFastMaxDeg, kFastMaxCnDeg, "the compile-time kernels"}
                        : kernel == KERNEL_GENERATED   ? KernelCases{tree_kind, true, INT32_MAX, INT32_MAX, "the generated kernel"}
                                                       : KernelCases{tree_kind, true, 255, 255, "the interpreter"};
    return validate_class(d, P, "class launch check failed, class " + std::to_string(i), k);
}

// One pass of the streaming decode: every degree class through the kernel pass_kernel names, one launch each (the classes of a
// pass own disjoint rows).  KIND = TT_CHK covers both check updates, min-sum and CHKTREE.
template <int KIND>
static int launch_pass(lutldpc_decoder *d, int set, int G, int nz, int check, int write_hard, int kind_id) {
    const bool minsum = KIND == TT_CHK && d->min_lut;
    const TreeSetPlan *S = minsum ? nullptr : d->tree_set(KIND, set);
    if (!minsum && (!S || !S->valid)) return fail(LUTLDPC_ERR_STATE, "no trees of this pass in this tree set");
    Timed t(d, kind_id);
    const PassBufs bufs = pass_bufs(d);
    for (size_t i = 0; i < (KIND == TT_CHK ? d->cclass : d->vclass).size(); i++) {
        const PassKernel k = pass_kernel(d, KIND, set, (int)i, nz);
        const ClassParams P = KIND != TT_CHK ? vn_class_params(d, KIND, set, i, {0, G}, nz, check, write_hard)
                              : minsum       ? cn_class_params(d, i, {0, G}, nz, check)
                                             : lut_cn_class_params(d, set, i, {0, G}, nz, check);
        if (int rc = check_class_launch(d, P, i, KIND, k)) return rc;
        DEV_PARAM(dP, d, P);
        if (k == KERNEL_FAST) {
            bool ok = false;
            if constexpr (KIND == TT_CHK) PACK_DISPATCH(d, ok = launch_cn_fast<PK>(d->stream, P, dP, bufs));
            else PACK_DISPATCH(d, ok = launch_vn_fast<KIND, PK>(d->stream, P, dP, bufs));
            if (!ok) return fail(LUTLDPC_ERR_STATE, "no compile-time kernel for degree " + std::to_string(P.deg));
        } else if (k == KERNEL_GENERATED) {
            void *args[] = {&dP, (void *)&bufs.msgs, (void *)&bufs.cha, (void *)&bufs.hard, (void *)&bufs.state_w, (void *)&bufs.vfail_w, (void *)&bufs.tables, (void *)&bufs.fast_idx};
            HIP_TRY(hipModuleLaunchKernel(S->cls[i].jit->fn, class_blocks(P), 1, 1, 256, 1, 1, 0, d->stream, args, nullptr));
        } else {                                                      // a block is one wave
            const dim3 grid((unsigned)(P.waves_per_group * P.G)), block(64);
            if (minsum) {
                PACK_DISPATCH(d, launch_k(cn_minsum_generic_kernel<PK>, grid, block, 0, d->stream, dP, bufs.msgs, bufs.state_w, bufs.vfail_w, bufs.fast_idx));
                continue;
            }
            const Program &pr = S->cls[i].base.prog;
            const int slot_bytes = interp_slot_bytes(pr);
            const bool lds_tab = slot_bytes + P.tab_len[0] <= 64 * 1024;
            const size_t lds = (size_t)(slot_bytes + (lds_tab ? P.tab_len[0] : 0));
            const Op *prog = d->d_ops.p + S->cls[i].op_off;
#define TREE_PASS(LDS_TAB) PACK_DISPATCH(d, launch_k(tree_pass_kernel<KIND, LDS_TAB, PK>, grid, block, lds, d->stream, dP, bufs.msgs, bufs.cha, bufs.hard, bufs.state_w, bufs.vfail_w, \
                                                  prog, bufs.tables, bufs.fast_idx, (int)pr.ops.size(), pr.n_slots, pr.n_out))
            if (lds_tab) TREE_PASS(true); else TREE_PASS(false);
#undef TREE_PASS
        }
    }
    LAUNCH_CHECK();
    return LUTLDPC_OK;
}

// Are the decided bits of early-terminated frames recovered at the end (hard_from_frozen_kernel) instead of being stored by
// every variable pass?  Min-sum checks, one message alphabet, and -- in the skewed pipeline -- chain fusion on in every
// iteration or in none (the nodes it updates get their bits from the check pass).  `chain_skip`: those nodes are skipped by
// the recovery.  (Compaction then moves the frozen rows of finished frames along: launch_compaction.)
bool late_hard_active(const lutldpc_decoder *d, bool skewed, bool *chain_skip) {
    if (chain_skip) *chain_skip = false;
    if (!d->opt.late_hard || !d->psc || !d->min_lut) return false;
    for (int i = 1; i < d->max_iters; i++) if (d->Nq_Msg[(size_t)i] != d->Nq_Msg[0]) return false;
    if (!skewed) return true;
    int on = 0, off = 0;
    for (int ii = 0; ii + 1 < d->max_iters; ii++) (chain_active(d, d->iter_set[(size_t)ii]) ? on : off)++;
    if (on && off) return false;
    if (chain_skip) *chain_skip = on > 0;
    return true;
}

// chain fusion applies to a check pass that is followed by a variable pass (not the last iteration) when the degree-2
// class has the compile-time kernel (its root table is staged)
bool chain_active(const lutldpc_decoder *d, int set) {
    if (!d->opt.use_chain || d->chain_vclass < 0 || d->n_chain_nodes == 0) return false;
    const TreeClassPlan *t = d->tree_class(TT_VAR, set, d->chain_vclass);
    return t && t->fast.ok && t->fast.n_tables == 1 && t->fast.tab_len[0] <= 1024;
}

// Decided bits of the frames that left through the exit test, read off their frozen messages (hard_from_frozen_kernel) and, for
// the nodes updated inside the check pass, off the parity equations (chain_hard_kernel): groups g0 .. g0+G-1, at the end of the decode.
int launch_late_hard(lutldpc_decoder *d, bool skewed, int g0, int G) {
    bool chain_skip = false;
    if (!late_hard_active(d, skewed, &chain_skip) || G <= 0) return LUTLDPC_OK;
    PACK_DISPATCH(d, launch_k(hard_from_frozen_kernel<PK>, dim3(std::min<unsigned>(2048u, (unsigned)((d->nvar + 3) / 4)), (unsigned)G), dim3(256), 0, d->stream, d->d_msgs.p, d->d_hard.p,
                                        reinterpret_cast<const uint32_t *>(d->d_state.p), d->d_vn_ptr.p, chain_skip ? d->d_chain_internal.p : nullptr, d->nvar, d->E,
                                        d->Nq_Msg[0] / 2, g0));
    if (chain_skip)
        for (size_t i = 0; i < d->cclass.size(); i++) {
            if (d->cclass[i].chain_off < 0) continue;
            const int n = (int)d->cclass[i].nodes.size(), npw = d->npw_cn_class(i), runs = (n + npw - 1) / npw;
            PACK_DISPATCH(d, launch_k(chain_hard_kernel<PK>, dim3(std::min<unsigned>(512u, (unsigned)((runs + 3) / 4)), (unsigned)G), dim3(256), 0, d->stream, d->d_hard.p,
                                                reinterpret_cast<const uint32_t *>(d->d_state.p), d->d_fast_idx.p + d->cclass[i].idx_off, d->d_fast_idx.p + d->cclass[i].chain_off,
                                                d->d_edge_vn.p, n, d->cclass[i].deg, npw, d->nvar, g0));
        }
    LAUNCH_CHECK();
    return LUTLDPC_OK;
}

// one message dump of the trace: the E edge rows of all frames, frame-major, to the next slot of the host buffer (synchronous)
static int trace_dump(lutldpc_decoder *d) {
    lutldpc_decoder::Trace &T = d->trace;
    if (T.hist) return hist_dump(d);               // the sink is a histogram on the device (decoder_stats.hip): nothing is copied
    const size_t one = (size_t)T.B * (size_t)d->E;
    if ((size_t)(T.n + 1) * one > T.cap) return fail(LUTLDPC_ERR_ARG, "trace buffer too small");
    // rows_to_host stages through d_out_bits, whose pointer the caller of this decode may hold already (decode_staged_labels sizes
    // it for a dump): never let it move here
    if (d->d_out_bits.n < one) return fail(LUTLDPC_ERR_STATE, "trace: the staging buffer was not sized for a dump");
    if (int rc = rows_to_host(d, d->d_msgs.p, T.host + (size_t)T.n * one, T.B, d->E)) return rc;
    HIP_TRY(hipStreamSynchronize(d->stream));
    T.n++;
    return LUTLDPC_OK;
}

// Core: decode the B frames whose labels are already in tile layout (d_cha_t / d_msg0_t).
// Leaves the decided bits in d_hard (tile layout) and the iteration codes in d_iters.
static int decode_tiles_launch(lutldpc_decoder *d, int B, const FrameMajorIO *fm = nullptr) {
    int rc;
    const int Bpad = d->bpad(B), G = Bpad / d->tile();
    const int N = d->nvar, E = d->E, I = d->max_iters;
    const int last_set = d->iter_set[(size_t)(I - 1)];
    if (!d->tree_set(TT_DEC, last_set)->valid)
        return fail(LUTLDPC_ERR_STATE, "the tree set of iteration max_iters-1 is not a decision tree set");
    if ((rc = launch_state(d, B, Bpad, 0, 0))) return rc;
    const bool tracing = d->trace.level > 1;
    if (resident_active(d) && !tracing) {         // the whole of lut_decode in one launch, messages in LDS (jit_resident.hpp)
        if ((rc = launch_resident(d, G, B, fm))) return rc;
        if (d->profiling && d->ev_live.size() > 8192) prof_fold(d);
        return LUTLDPC_OK;
    }
    if (d->pisc) {   // :275-279
        if (is_pow2(d->Nq_Cha / 2)) {
            if ((rc = launch_syndrome_of_labels(d, G))) return rc;
        } else {
            // the decided bit `label < Nq_Cha/2` is the inverted sign BIT of the label only when Nq_Cha/2 is a power of two: any other
            // channel alphabet goes through decided-bit rows (SWAR compare) and the parity pass over them
            {
                Timed t(d, LUTLDPC_K_LAYOUT);
                const size_t n_words = (size_t)G * (size_t)N * kRowBytes / 4;
                PACK_DISPATCH(d, launch_k(hard_from_labels_kernel<PK>, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, d->stream, d->d_cha_t.p, d->d_hard.p, n_words, d->Nq_Cha / 2));
                LAUNCH_CHECK();
            }
            if ((rc = launch_syndrome(d, G))) return rc;
        }
        if ((rc = launch_state(d, B, Bpad, 1, 0))) return rc;
        {   // decided bits of the frames that passed = signs of their channel labels (:275); groups without such a frame return at once
            Timed t(d, LUTLDPC_K_LAYOUT);
            PACK_DISPATCH(d, launch_k(hard_from_labels_masked_kernel<PK>, dim3(std::min<unsigned>(1024u, (unsigned)((N + 3) / 4)), (unsigned)G), dim3(256), 0, d->stream,
                                                d->d_cha_t.p, d->d_hard.p, reinterpret_cast<const uint32_t *>(d->d_state.p), N, d->Nq_Cha / 2, 0));
            LAUNCH_CHECK();
        }
    }
    const bool skewed = d->opt.skew && d->skew_ok && !tracing;      // (a single frame group runs the same launches with an empty second half)
    if (!(skewed && d->opt.first_from_nodes)) {   // :284-289 (the fused pipeline's first check pass reads the initial-message rows itself)
        Timed t(d, LUTLDPC_K_LAYOUT);
        launch_k(init_edges_kernel, dim3((unsigned)((N + 3) / 4), (unsigned)G), dim3(256), 0, d->stream, d->d_msg0_t.p, d->d_msgs.p, d->d_vn_ptr.p, N, E);
        LAUNCH_CHECK();
    }
    if (tracing && (rc = trace_dump(d))) return rc;                              // :292-298
    if (skewed && (rc = iterate_skewed(d, B, Bpad, G))) return rc;
    for (int ii = 0; ii < I && !skewed; ii++) {   // :301-338
        const int set = d->iter_set[(size_t)ii];
        const int nz_in = d->Nq_Msg[(size_t)ii] / 2;
        const int chk_check = (d->psc && ii > 0) ? 1 : 0;    // finishes the test started by VN pass ii-1
        if ((rc = launch_pass<TT_CHK>(d, set, G, nz_in, chk_check, 0, LUTLDPC_K_CN_PASS))) return rc;
        if (chk_check && (rc = launch_state(d, B, Bpad, 2, ii))) return rc;   // :327-329 returns (ii-1)+1
        if (d->trace.level > 2 && (rc = trace_dump(d))) return rc;             // :311-317
        if (ii != I - 1) {
            const int nz_out = d->Nq_Msg[(size_t)(ii + 1)] / 2;
            rc = launch_pass<TT_VAR>(d, set, G, nz_out, d->psc ? 1 : 0, (d->psc && !late_hard_active(d, false, nullptr)) ? 1 : 0, LUTLDPC_K_VN_PASS);
            if (rc) return rc;
        }
        if (tracing && (rc = trace_dump(d))) return rc;                         // :331-337 (printed after the last iteration too)
    }
    if (d->trace.hist) {                            // a counted decode ends with its last dump: bits and iteration codes are those of the decode before it
        if (d->profiling && d->ev_live.size() > 8192) prof_fold(d);
        return LUTLDPC_OK;
    }
    {   // decided bits of the frames that left through the exit test, from their frozen messages (see late_hard_active)
        Timed t(d, LUTLDPC_K_LAYOUT);
        if ((rc = launch_late_hard(d, skewed, 0, G))) return rc;
        if (skewed && d->psc && d->pisc && compaction_on(d, G) && late_hard_active(d, true, nullptr)) {
            // frames that passed the test on the channel decisions may have been moved by a permutation: their decided-bit rows
            // did not travel (no other decided bit exists during the iterations), their channel rows did -- write the bits again
            PACK_DISPATCH(d, launch_k(hard_from_labels_masked_kernel<PK>, dim3(std::min<unsigned>(1024u, (unsigned)((N + 3) / 4)), (unsigned)G), dim3(256), 0, d->stream,
                                                d->d_cha_t.p, d->d_hard.p, reinterpret_cast<const uint32_t *>(d->d_state.p), N, d->Nq_Cha / 2, 0));
            LAUNCH_CHECK();
        }
    }
    // :340-349
    if ((rc = launch_pass<TT_DEC>(d, last_set, G, 0, 0, 0, LUTLDPC_K_DECISION))) return rc;
    const int fsel = skewed ? (I & 1) : 0;            // the flag buffer no pass of the skewed pipeline has written since its last test
    if ((rc = launch_syndrome(d, G, fsel))) return rc;
    if ((rc = launch_state(d, B, Bpad, 3, I, 0, -1, fsel))) return rc;
    if (skewed && d->psc && compaction_on(d, G)) {
        const HalfRange half[2] = {{0, (G + 1) / 2}, {(G + 1) / 2, G - (G + 1) / 2}};
        if ((rc = launch_uncompaction(d, half, Bpad))) return rc;
    }
    if (d->profiling && d->ev_live.size() > 8192) prof_fold(d);
    return LUTLDPC_OK;
}

// A decode is 100-300 short launches whose arguments depend only on (B, exit conditions): from the
// second call with the same key on, the sequence is replayed as ONE hipGraph launch (the first call runs
// plainly and fills the item-table cache, whose uploads may not happen inside a capture).  Short codes
// are launch-bound, for them this is worth ~20 %.  Off while kernel events are being recorded.
int decode_tiles(lutldpc_decoder *d, int B, const FrameMajorIO *fm) {
    if (int rc = check_batch_buffers(d, d->bpad(B))) return rc;
    if (resident_active(d) && !d->trace.hist) {   // generate / compile / load outside any stream capture (a counted decode streams)
        lutldpc_decoder::ResidentPlan *pl = nullptr;
        if (int rc = resident_plan_for(d, d->bpad(B) / d->tile(), &pl)) return rc;
    }
    // (the resident decoder is ONE launch plus the state kernel: nothing to gain from a graph.  It is never captured into one, which
    // is why a caller's frame-major pointers, fm, may enter its launch: a graph would freeze them.  No other path reads fm.)
    if (!d->opt.use_graph || d->profiling || d->trace.level > 1 || resident_active(d)) return decode_tiles_launch(d, B, fm);
    const std::array<int, 4> key = {B, d->psc, d->pisc, d->max_iters};
    if (d->graphs.size() > 32 && !d->graphs.count(key)) d->drop_graphs();      // callers with ever-changing batch sizes: bound the cache
    auto &slot = d->graphs[key];
    if (slot.exec) {
        HIP_TRY(hipGraphLaunch(slot.exec, d->stream));
        return LUTLDPC_OK;
    }
    if (slot.seen++ == 0) return decode_tiles_launch(d, B);
    HIP_TRY(hipStreamBeginCapture(d->stream, hipStreamCaptureModeThreadLocal));
    const int rc = decode_tiles_launch(d, B);
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(d->stream, &g);
    if (rc || e != hipSuccess || !g) {
        if (g) (void)hipGraphDestroy(g);
        (void)hipGetLastError();
        d->opt.use_graph = 0;                             // capture not possible here: plain launches from now on
        return rc ? rc : decode_tiles_launch(d, B);
    }
    const hipError_t ei = hipGraphInstantiate(&slot.exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (ei != hipSuccess) { slot.exec = nullptr; d->opt.use_graph = 0; (void)hipGetLastError(); return decode_tiles_launch(d, B); }
    HIP_TRY(hipGraphLaunch(slot.exec, d->stream));
    return LUTLDPC_OK;
}

// The batched lut_decode (src/LDPC_Code_LUT.cpp:259-353) on device-resident frame-major labels (after the entry's batch_entry).
int decode_device(lutldpc_decoder *d, const uint8_t *d_cha, const uint8_t *d_msg0, int B, uint8_t *d_out_bits) {
    // the LDS-resident decoder reads the frame-major labels and writes the frame-major bits itself
    const bool direct = resident_active(d) && d->opt.resident_fm && d->trace.level <= 1;
    int rc = direct ? ensure_batch(d, B) : tiles_from_device(d, d_cha, d_msg0, B);
    if (rc) return rc;
    const FrameMajorIO fm = {d_cha, d_msg0, d_out_bits};
    if ((rc = decode_tiles(d, B, direct ? &fm : nullptr)) || direct) return rc;
    Timed t(d, LUTLDPC_K_LAYOUT);
    return launch_transpose_out(d, d->d_hard.p, d_out_bits, B, d->bpad(B) / d->tile());
}

#pragma GCC visibility pop
