// decoder_skew.hip -- the skewed two-half pipeline through pass_fused_kernel and the compaction of the surviving frames.
// Home of every kernel of kernels_compact.hpp.
#include "decoder_state.hpp"
#include "kernels_compact.hpp"

#pragma GCC visibility push(hidden)

// ----------------------------------------------------------------------------- skewed two-half pipeline
// (kernels_fast.hpp: pass_fused_kernel).  Half A = groups [0, GA), half B = [GA, G).  Each half runs
// the reference's sequence  CN(0) VN(0) CN(1) ... CN(I-1)  (src/LDPC_Code_LUT.cpp:301-338); B lags A by
// one pass, so every launch pairs a check pass of one half with a variable pass of the other.

bool skew_eligible(const lutldpc_decoder *d) {
    if (!d->min_lut || !d->opt.use_fast) return false;
    if ((int)(d->cclass.size() + d->vclass.size()) > kFusedMaxRoles) return false;
    int max_cn = 0, max_vn = 0;
    for (auto &c : d->cclass) { if (c.deg < 2) return false; max_cn = std::max(max_cn, c.deg); }
    for (auto &c : d->vclass) max_vn = std::max(max_vn, c.deg);
    if (fused_bucket(max_vn, max_cn) < 0) return false;
    for (int nq : d->Nq_Msg) if (!is_pow2(nq / 2) || nq / 2 > 64) return false;
    for (size_t s = 0; s < d->var_fast.size(); s++) {
        if (d->var_plan[s].valid == false) continue;          // decision-only set
        for (auto &f : d->var_fast[s])
            if (!f.ok || f.P.n_tables > kFusedMaxTables) return false;
    }
    return true;
}

static void add_cn_roles(const lutldpc_decoder *d, FusedParams &FP, std::vector<int> &blocks, HalfRange h, int ii, int check) {
    const int I = d->max_iters, nz = d->Nq_Msg[(size_t)ii] / 2;
    const int buf_w = kVfailSlots * d->Bcap / 4;                      // words per flag buffer
    const bool on = ii != I - 1 && chain_active(d, d->iter_set[(size_t)ii]);
    // decided bits of the nodes updated here: stored by the check pass that reads their messages, unless they are recovered at
    // the end with everything else (late_hard_active + chain_hard_kernel)
    const bool hard = d->psc && ii >= 1 && chain_active(d, d->iter_set[(size_t)(ii - 1)]) && !late_hard_active(d, true, nullptr);
    for (size_t i = 0; i < d->cclass.size(); i++) {
        RoleParams R{};
        R.vfail_off_w = (ii & 1) * buf_w;                             // parity flags: this iteration's exit test
        if ((on || hard) && d->chain_idx_off[i] >= 0) {
            R.chain.idx_off = d->chain_idx_off[i];
            R.chain.hard = hard ? 1 : 0;
            if (on) {
                const FastParams &F2 = d->var_fast[(size_t)d->iter_set[(size_t)ii]][(size_t)d->chain_vclass].P;
                R.chain.on = 1;
                R.chain.tab_off = F2.tab_off[0]; R.chain.tab_len = F2.tab_len[0]; R.chain.tab_shift = F2.tab_shift[0];
                R.chain.check = d->psc ? 1 : 0;
                R.chain.vfail_off_w = ((ii + 1) & 1) * buf_w;         // unanimity of the nodes updated here: the next exit test
                R.chain.sbit_out = __builtin_ctz((unsigned)(d->Nq_Msg[(size_t)(ii + 1)] / 2) | 0x100u);
            }
        }
        const int npw = d->npw_cn_class(i);
        R.kind = 0; R.deg = d->cclass[i].deg; R.g0 = h.g0; R.G = h.G;
        R.n_nodes = (int)d->cclass[i].nodes.size(); R.nodes_per_wave = npw;
        R.waves_per_group = (R.n_nodes + npw - 1) / npw;
        R.idx_off = d->cn_idx_off[i]; R.E = d->E; R.N = d->nvar; R.nz = nz; R.check = check; R.vfail_stride_w = d->Bcap / 4;
        if (ii == 0 && d->opt.first_from_nodes) { R.first = 1; R.nidx_off = d->cn_nidx_off[i]; }
        FP.role[FP.n_roles++] = R;
        blocks.push_back((R.waves_per_group * h.G + 3) / 4);
    }
}
static void add_vn_roles(const lutldpc_decoder *d, FusedParams &FP, std::vector<int> &blocks, HalfRange h, int ii, int check, int write_hard) {
    const int set = d->iter_set[(size_t)ii], nz = d->Nq_Msg[(size_t)(ii + 1)] / 2;
    const bool chained = chain_active(d, set);
    const int buf_w = kVfailSlots * d->Bcap / 4;
    for (size_t i = 0; i < d->vclass.size(); i++) {
        const FastParams &F = d->var_fast[(size_t)set][i].P;
        const int npw = d->npw_vn(F.deg);
        RoleParams R{};
        R.kind = 1; R.deg = F.deg; R.g0 = h.g0; R.G = h.G;
        R.n_nodes = F.n_nodes; R.nodes_per_wave = npw;
        R.idx_off = F.idx_off;
        if (chained && (int)i == d->chain_vclass) { R.n_nodes = d->vn_red_n[i]; R.idx_off = d->vn_red_off[i]; }   // the others were updated by the check pass
        R.waves_per_group = (R.n_nodes + npw - 1) / npw; R.E = d->E; R.N = d->nvar; R.nz = nz; R.shift_msg = F.shift_msg; R.check = check; R.write_hard = write_hard; R.vfail_stride_w = d->Bcap / 4;
        R.vfail_off_w = ((ii + 1) & 1) * buf_w;                       // unanimity flags: the exit test after the NEXT check pass
        for (int t = 0; t < F.n_tables; t++) { R.tab_off[t] = F.tab_off[t]; R.tab_len[t] = F.tab_len[t]; R.tab_shift[t] = F.tab_shift[t]; }
        FP.role[FP.n_roles++] = R;
        blocks.push_back((R.waves_per_group * h.G + 3) / 4);
    }
}

// interleave the blocks of all roles evenly over the launch: block j of a role with n blocks sits at
// position (j + 1/2) / n of the timeline
static int item_table(lutldpc_decoder *d, const std::vector<int> &blocks, const std::vector<double> &front, const int32_t **out, int *total) {
    int nb = 0;
    for (int b : blocks) nb += b;
    *total = nb;
    std::vector<int> fq(front.size());
    for (size_t r = 0; r < front.size(); r++) fq[r] = (int)(front[r] * 4096.0);
    const auto key = std::make_pair(blocks, fq);
    auto it = d->item_tabs.find(key);
    if (it == d->item_tabs.end()) {
        std::vector<std::pair<double, std::pair<int, int>>> pos;
        pos.reserve((size_t)nb);
        // `front[r]` in [0,1): roles with long-running blocks are issued over [0, 1 - front) only, so that the
        // launch does not end on a tail of a few slow blocks (the next launch needs this one complete)
        for (size_t r = 0; r < blocks.size(); r++)
            for (int j = 0; j < blocks[r]; j++) pos.push_back({((double)j + 0.5) / (double)blocks[r] * (1.0 - front[r]), {(int)r, j}});
        std::stable_sort(pos.begin(), pos.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
        std::vector<int32_t> h;
        h.reserve(2 * (size_t)nb);
        for (auto &q : pos) { h.push_back(q.second.first); h.push_back(q.second.second); }
        DevBuf<int32_t> buf;
        HIP_TRY(buf.upload(h));
        it = d->item_tabs.emplace(key, std::move(buf)).first;
    }
    *out = it->second.p;
    return LUTLDPC_OK;
}

// LUTLDPC_VALIDATE: the roles of one fused launch against the sizes of everything they address
static int validate_fused(const lutldpc_decoder *d, const FusedParams &FP, const std::vector<int> &blocks) {
    auto bad = [&](int r, const std::string &what) { return fail(LUTLDPC_ERR_STATE, "fused launch check failed, role " + std::to_string(r) + ": " + what); };
    if (FP.n_roles < 0 || FP.n_roles > kFusedMaxRoles || (size_t)FP.n_roles != blocks.size()) return bad(-1, "role count");
    const int groups = d->Bcap / d->tile();
    const size_t idx_n = d->fast_idx.size(), tab_n = d->d_tables.n, vfail_w = d->d_vfail.n / 4;
    for (int r = 0; r < FP.n_roles; r++) {
        const RoleParams &R = FP.role[r];
        if (R.G < 1 || R.g0 < 0 || R.g0 + R.G > groups) return bad(r, "frame groups outside the batch buffers");
        if (R.E != d->E || R.N != d->nvar) return bad(r, "E / N");
        if (R.n_nodes < 1 || R.nodes_per_wave < 1 || R.waves_per_group != (R.n_nodes + R.nodes_per_wave - 1) / R.nodes_per_wave) return bad(r, "waves per group");
        if (blocks[(size_t)r] != (R.waves_per_group * R.G + 3) / 4) return bad(r, "block count");
        if (R.vfail_stride_w != d->Bcap / 4 || R.vfail_off_w < 0 || (size_t)R.vfail_off_w + (size_t)kVfailSlots * (size_t)R.vfail_stride_w > vfail_w) return bad(r, "flag buffer");
        if (R.kind == 0) {
            if (R.deg < 2 || R.deg > kFusedCnDeg[d->fused_bucket_id]) return bad(r, "check degree outside the bucket");
            if (R.idx_off < 0 || (size_t)R.idx_off + (size_t)R.n_nodes * (size_t)R.deg > idx_n) return bad(r, "edge table");
            if (!is_pow2(R.nz) || R.nz > 64) return bad(r, "nz");
            if (R.first && (R.nidx_off < 0 || (size_t)R.nidx_off + (size_t)R.n_nodes * (size_t)R.deg > idx_n || R.check || R.chain.hard)) return bad(r, "node table of the first check pass");
            if (R.chain.on || R.chain.hard) {
                if (R.chain.idx_off < 0 || (size_t)R.chain.idx_off + 2 * (size_t)R.n_nodes > idx_n) return bad(r, "chain link table");
                if (R.chain.on && (R.chain.tab_off < 0 || R.chain.tab_len < 4 || R.chain.tab_len > 1024 || (size_t)R.chain.tab_off + (size_t)R.chain.tab_len > tab_n)) return bad(r, "chain table");
                if (R.chain.on && R.chain.check && (R.chain.vfail_off_w < 0 || (size_t)R.chain.vfail_off_w + (size_t)kVfailSlots * (size_t)R.vfail_stride_w > vfail_w)) return bad(r, "chain flag buffer");
            }
        } else {
            if (R.deg < 1 || R.deg > kFusedVnDeg[d->fused_bucket_id]) return bad(r, "variable degree outside the bucket");
            if (R.idx_off < 0 || (size_t)R.idx_off + 2 * (size_t)R.n_nodes > idx_n) return bad(r, "node table");
            const int nt = R.deg >= 3 ? R.deg - 1 : 1;
            for (int t = 0; t < nt; t++)
                if (R.tab_off[t] < 0 || R.tab_len[t] < 1 || R.tab_len[t] > kFastTableStride || (R.tab_off[t] & 3) || (size_t)R.tab_off[t] + (size_t)R.tab_len[t] > tab_n) return bad(r, "table " + std::to_string(t));
        }
    }
    return LUTLDPC_OK;
}

// the item table of one launch: per-wave work of a role ~ edges per wave, a variable-node edge costing about 3x a check
// edge (LUT look-ups); the slow roles keep clear of the end of the launch (item_table)
static int plan_items(lutldpc_decoder *d, const FusedParams &FP, const std::vector<int> &blocks, const int32_t **items, int *nb) {
    std::vector<double> cost(blocks.size()), front(blocks.size());
    double cmax = 0;
    for (size_t r = 0; r < blocks.size(); r++) {
        const RoleParams &R = FP.role[r];
        cost[r] = (double)R.deg * R.nodes_per_wave * (R.kind ? 3.0 * R.deg / 4.0 : 1.0);
        cmax = std::max(cmax, cost[r]);
    }
    for (size_t r = 0; r < blocks.size(); r++) front[r] = d->opt.tail_front * cost[r] / (cmax > 0 ? cmax : 1.0);
    return item_table(d, blocks, front, items, nb);
}

static int launch_fused_slot(lutldpc_decoder *d, const lutldpc_decoder::SkewPlan &plan, const lutldpc_decoder::SkewSlot &sl, bool vn_check) {
    if (sl.nb == 0) return LUTLDPC_OK;
    Timed t(d, LUTLDPC_K_FUSED_PASS);
#define FUSED_ARGS d->stream, plan.d_roles.p + sl.role_off, sl.items, sl.nb, d->opt.fused_prio, vn_check, d->d_msgs.p, d->d_cha_t.p, d->d_hard.p, \
                   reinterpret_cast<const uint32_t *>(d->d_state.p), reinterpret_cast<uint32_t *>(d->d_vfail.p), d->d_tables.p, d->d_fast_idx.p, d->d_msg0_t.p
    if (d->fused_bucket_id == 0) PACK_DISPATCH(d, (lutldpc::launch_fused<PK, 0>(FUSED_ARGS)));
    else if (d->fused_bucket_id == 1) PACK_DISPATCH(d, (lutldpc::launch_fused<PK, 1>(FUSED_ARGS)));
    else if (d->fused_bucket_id == 2) PACK_DISPATCH(d, (lutldpc::launch_fused<PK, 2>(FUSED_ARGS)));
    else PACK_DISPATCH(d, (lutldpc::launch_fused<PK, 3>(FUSED_ARGS)));
#undef FUSED_ARGS
    LAUNCH_CHECK();
    if (d->opt.validate) {                               // attribute a device fault to this launch
        hipError_t e = hipStreamSynchronize(d->stream);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) return fail(LUTLDPC_ERR_HIP, std::string("fused launch failed on the device: ") + hipGetErrorString(e));
    }
    return LUTLDPC_OK;
}

// kernels_compact.hpp: a check point of one half right after its exit test of iteration ii -- the plan kernel decides on the
// device whether permuting the slots (active frames first) pays; if not, the row kernels return at once
constexpr unsigned kPermuteBlocks = 512;      // two 16-wave blocks per CU
static bool compaction_fits(const lutldpc_decoder *, int GH) { return GH <= kPermuteMaxGroups; }
// A check point costs three short launches per half (~15 us) whether it permutes or not: automatic mode switches compaction on
// only where one iteration of the batch lasts long enough to make that noise (estimated from its row traffic at 5.5 TB/s);
// LUTLDPC_COMPACT=1 / 0 forces it on / off.  (Measured on MI355X it does not pay on the benchmark workloads: DVB-S2 frames finish
// too late -- 41.7 of 50 iterations on average --, (3,6) frames finish so close together that whole groups fall idle by themselves.)
bool compaction_on(const lutldpc_decoder *d, int G) {
    if (!compaction_fits(d, (G + 1) / 2) || G < 4) return false;
    if (d->opt.use_compact >= 0) return d->opt.use_compact != 0;
    const double est_iter_us = (4.0 * d->E + 3.0 * d->nvar) * kRowBytes * G / 5.5e6;
    return est_iter_us >= 400.0;
}
int compaction_min_groups(const lutldpc_decoder *d) {
    for (int G = 1; G <= 2 * kPermuteMaxGroups; G++) if (compaction_on(d, G)) return G;
    return -1;
}
// (see preload_code_objects) this unit's code object, and the 66 KB of dynamic LDS the row permutation uses (kernels_compact.hpp)
hipError_t preload_compact_kernels() {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&permute_rows_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, kPermuteLdsBytes);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(&permute_rows_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, kPermuteLdsBytes);
}
static int launch_compaction(lutldpc_decoder *d, HalfRange h, int hf, int ii) {
    Timed t(d, LUTLDPC_K_LAYOUT);
    const int T = d->tile(), s0 = h.g0 * T, n = h.G * T;
    if (n <= 0) return LUTLDPC_OK;
    uint8_t *pending = d->d_vfail.p + (size_t)((ii + 1) & 1) * kVfailSlots * d->Bcap;      // flags already raised for the next test
    int32_t *ctl = d->d_ctl.p + 4 * hf;
    const bool late = late_hard_active(d, true, nullptr);
    // keep: the frames that left keep their frozen rows (moved behind the active ones), their decided bits are recovered once
    // at the end of the decode like without compaction; otherwise (LUTLDPC_COMPACT_KEEP=0) they are recovered at the check point
    // and the rows dropped
    const bool keep = late && d->opt.compact_keep;
    launch_k(compact_decide_kernel, dim3(1), dim3(1024), 0, d->stream, d->d_state.p, s0, n, T, ctl, d->max_iters - 1 - ii, (float)d->opt.compact_margin,
                       d->opt.compact_margin > 0 ? (float)d->opt.compact_min_share : 0.0f, keep ? 1 : 0);
    // (not keep) the decided bits of the frames that left since the last permutation, before their messages are dropped
    if (!keep) if (int rc = launch_late_hard(d, true, h.g0, h.G, ctl)) return rc;
    launch_k(compact_apply_kernel, dim3(1), dim3(1024), 0, d->stream, d->d_state.p, d->d_iters.p, d->d_frame_of.p, pending, d->Bcap, s0, n,
                       d->d_perm.p, d->d_tmp3.p + (size_t)3 * s0, ctl, (late && !keep) ? 1 : 0);
    // (the grid is fixed and small: an empty check point must cost microseconds)
    auto rows = [&](uint8_t *a, int na, uint8_t *b, int nb, int gather) {
        const unsigned blocks = std::min<unsigned>(kPermuteBlocks, (unsigned)((na + nb + kPermuteRows - 1) / kPermuteRows));
        PACK_DISPATCH(d, launch_k(permute_rows_kernel<PK>, dim3(blocks), dim3(1024), kPermuteLdsBytes, d->stream, a, na, b, nb, h.g0, h.G,
                                            d->d_perm.p, d->d_ctl.p + 4 * hf, gather));
    };
    rows(d->d_msgs.p, d->E, d->d_cha_t.p, d->nvar, keep ? 2 : 1);
    if (!keep) rows(d->d_hard.p, d->nvar, nullptr, 0, 0);        // (keep: no decided bit exists before the end of the decode)
    LAUNCH_CHECK();
    return LUTLDPC_OK;
}
// end of the decode: decided bits and iteration codes back into the caller's frame order
int launch_uncompaction(lutldpc_decoder *d, const HalfRange (&half)[2], int Bpad) {
    Timed t(d, LUTLDPC_K_LAYOUT);
    launch_k(invert_map_kernel, dim3((unsigned)((Bpad + 255) / 256)), dim3(256), 0, d->stream, d->d_frame_of.p, d->d_slot_of.p, 0, Bpad);
    for (int hf = 0; hf < 2; hf++) {
        if (half[hf].G <= 0) continue;
        PACK_DISPATCH(d, launch_k(permute_rows_kernel<PK>, dim3(std::min<unsigned>(kPermuteBlocks, (unsigned)((d->nvar + kPermuteRows - 1) / kPermuteRows))), dim3(1024),
                                            kPermuteLdsBytes, d->stream, d->d_hard.p, d->nvar, (uint8_t *)nullptr, 0,
                                            half[hf].g0, half[hf].G, d->d_slot_of.p, (const int32_t *)nullptr, 0));
    }
    launch_k(gather_i32_kernel, dim3((unsigned)((Bpad + 255) / 256)), dim3(256), 0, d->stream, d->d_iters.p, d->d_slot_of.p, d->d_iters_tmp.p, 0, Bpad);
    HIP_TRY(hipMemcpyAsync(d->d_iters.p, d->d_iters_tmp.p, sizeof(int32_t) * (size_t)Bpad, hipMemcpyDeviceToDevice, d->stream));
    LAUNCH_CHECK();
    return LUTLDPC_OK;
}

// Build (once per shape) the launch plan of the message-passing iterations of both halves: slot s pairs pass s of half A
// with pass s-1 of half B, a pass being CN(ii) for even and VN(ii) for odd numbers.  Every role is checked against the
// sizes of what it addresses before the plan is accepted (validate_fused), the roles then move to device memory once.
static int build_skew_plan(lutldpc_decoder *d, int G, lutldpc_decoder::SkewPlan &plan) {
    const int I = d->max_iters, n_ops = 2 * I - 1;
    const HalfRange half[2] = {{0, (G + 1) / 2}, {(G + 1) / 2, G - (G + 1) / 2}};
    const int psc = d->psc ? 1 : 0;
    int rc;
    for (int slot = 0; slot <= n_ops; slot++) {
        FusedParams FP{};
        std::vector<int> blocks;
        lutldpc_decoder::SkewSlot sl;
        for (int hf = 0; hf < 2; hf++) {
            const int op = slot - hf;                 // B lags by one pass
            if (op < 0 || op >= n_ops) continue;
            const int ii = op / 2;
            if ((op & 1) == 0) {                      // CN(ii)
                const int check = (psc && ii > 0) ? 1 : 0;
                add_cn_roles(d, FP, blocks, half[hf], ii, check);
                if (check) { sl.state_half = hf; sl.state_ii = ii; }
            } else {                                  // VN(ii)
                add_vn_roles(d, FP, blocks, half[hf], ii, psc, (psc && !late_hard_active(d, true, nullptr)) ? 1 : 0);
            }
        }
        // roles without work (an empty half when G == 1 never gets here; a degree class emptied by chain fusion does)
        FusedParams FQ{};
        std::vector<int> bq;
        for (int r = 0; r < FP.n_roles; r++) if (blocks[(size_t)r] > 0) { FQ.role[FQ.n_roles++] = FP.role[r]; bq.push_back(blocks[(size_t)r]); }
        if ((rc = validate_fused(d, FQ, bq))) return rc;
        if ((rc = plan_items(d, FQ, bq, &sl.items, &sl.nb))) return rc;
        sl.n_roles = FQ.n_roles; sl.role_off = plan.h_roles.size();
        plan.h_roles.insert(plan.h_roles.end(), FQ.role, FQ.role + FQ.n_roles);
        plan.slots.push_back(sl);
    }
    HIP_TRY(plan.d_roles.upload(plan.h_roles));
    return LUTLDPC_OK;
}

// the message-passing iterations of decode_tiles for both halves
int iterate_skewed(lutldpc_decoder *d, int B, int Bpad, int G) {
    const int I = d->max_iters;
    const HalfRange half[2] = {{0, (G + 1) / 2}, {(G + 1) / 2, G - (G + 1) / 2}};
    const int psc = d->psc ? 1 : 0;
    int rc;
    auto &pp = d->skew_plans[{G, psc, I}];
    if (!pp) {
        std::unique_ptr<lutldpc_decoder::SkewPlan> np(new lutldpc_decoder::SkewPlan());
        if ((rc = build_skew_plan(d, G, *np))) { d->skew_plans.erase({G, psc, I}); return rc; }
        pp = std::move(np);
    }
    const lutldpc_decoder::SkewPlan &plan = *pp;
    // compaction of the surviving frames: check points every `every` iterations (a check point costs three short launches
    // per half: keep that below a few per cent of an iteration, whose duration is estimated from its row traffic)
    const bool compact = psc && compaction_on(d, G);
    const int every = d->opt.compact_every > 0 ? d->opt.compact_every : 2;
    if (compact) {
        Timed t(d, LUTLDPC_K_LAYOUT);
        launch_k(compact_init_kernel, dim3((unsigned)((Bpad + 255) / 256)), dim3(256), 0, d->stream, d->d_frame_of.p, Bpad, d->d_ctl.p, half[0].G, half[1].G);
        LAUNCH_CHECK();
    }
    for (const auto &sl : plan.slots) {
        if ((rc = launch_fused_slot(d, plan, sl, psc != 0))) return rc;
        if (sl.state_half >= 0) {                     // :327-329 returns (ii-1)+1
            const int f0 = half[sl.state_half].g0 * d->tile(), f1 = f0 + half[sl.state_half].G * d->tile();
            if ((rc = launch_state(d, B, Bpad, 2, sl.state_ii, f0, f1, sl.state_ii & 1))) return rc;
            if (compact && sl.state_ii >= d->opt.compact_first && sl.state_ii < I - 2 && (sl.state_ii - d->opt.compact_first) % every == 0 &&
                (rc = launch_compaction(d, half[sl.state_half], sl.state_half, sl.state_ii))) return rc;
        }
    }
    return LUTLDPC_OK;
}

#pragma GCC visibility pop
