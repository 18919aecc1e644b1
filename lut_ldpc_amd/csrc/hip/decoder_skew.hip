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
    for (auto &c : d->cclass) max_cn = std::max(max_cn, c.deg);
    for (auto &c : d->vclass) max_vn = std::max(max_vn, c.deg);
    if (fused_bucket(max_vn, max_cn) < 0) return false;
    // every class on its compile-time kernel in every iteration (a balanced tree of a degree the bucket holds fits its table slots in LDS)
    for (int ii = 0; ii < d->max_iters_created; ii++) {
        const int set = d->iter_set[(size_t)ii];
        for (size_t i = 0; i < d->cclass.size(); i++) if (pass_kernel(d, TT_CHK, set, (int)i, d->Nq_Msg[(size_t)ii] / 2) != KERNEL_FAST) return false;
        if (ii + 1 == d->max_iters_created || !d->tree_set(TT_VAR, set)->valid) continue;      // (a decision-only set has no variable classes)
        for (size_t i = 0; i < d->vclass.size(); i++) if (pass_kernel(d, TT_VAR, set, (int)i, d->Nq_Msg[(size_t)ii + 1] / 2) != KERNEL_FAST) return false;
    }
    return true;
}

// the roles of pass ii of one half: every class with work (a degree class emptied by chain fusion has none)
static void add_cn_roles(const lutldpc_decoder *d, std::vector<ClassParams> &roles, HalfRange h, int ii, int check) {
    for (size_t i = 0; i < d->cclass.size(); i++) {
        const ClassParams R = cn_class_params(d, i, h, d->Nq_Msg[(size_t)ii] / 2, check, ii);
        if (class_blocks(R) > 0) roles.push_back(R);
    }
}
static void add_vn_roles(const lutldpc_decoder *d, std::vector<ClassParams> &roles, HalfRange h, int ii, int check, int write_hard) {
    for (size_t i = 0; i < d->vclass.size(); i++) {
        const ClassParams R = vn_class_params(d, TT_VAR, d->iter_set[(size_t)ii], i, h, d->Nq_Msg[(size_t)(ii + 1)] / 2, check, write_hard, ii);
        if (class_blocks(R) > 0) roles.push_back(R);
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

// the item table of one launch: per-wave work of a role ~ edges per wave, a variable-node edge costing about 3x a check
// edge (LUT look-ups); the slow roles keep clear of the end of the launch (item_table)
static int plan_items(lutldpc_decoder *d, const std::vector<ClassParams> &roles, const int32_t **items, int *nb) {
    std::vector<int> blocks(roles.size());
    std::vector<double> cost(roles.size()), front(roles.size());
    double cmax = 0;
    for (size_t r = 0; r < roles.size(); r++) {
        const ClassParams &R = roles[r];
        blocks[r] = (int)class_blocks(R);
        cost[r] = (double)R.deg * R.nodes_per_wave * (R.kind ? 3.0 * R.deg / 4.0 : 1.0);
        cmax = std::max(cmax, cost[r]);
    }
    for (size_t r = 0; r < roles.size(); r++) front[r] = d->opt.tail_front * cost[r] / (cmax > 0 ? cmax : 1.0);
    return item_table(d, blocks, front, items, nb);
}

static int launch_fused_slot(lutldpc_decoder *d, const lutldpc_decoder::SkewPlan &plan, const lutldpc_decoder::SkewSlot &sl, bool vn_check) {
    if (sl.nb == 0) return LUTLDPC_OK;
    Timed t(d, LUTLDPC_K_FUSED_PASS);
#define FUSED_ARGS d->stream, plan.d_roles.p + sl.role_off, sl.items, sl.nb, d->opt.fused_prio, vn_check, pass_bufs(d)
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
    // keep (the decided bits are recovered late): the frames that left keep their frozen rows, moved behind the active ones, and
    // their bits are recovered once at the end of the decode like without compaction.  Otherwise every variable pass has stored
    // the bits already: only the active frames' rows move, the decided-bit rows are permuted along, the rest is dropped
    const bool keep = late_hard_active(d, true, nullptr);
    launch_k(compact_decide_kernel, dim3(1), dim3(1024), 0, d->stream, d->d_state.p, s0, n, T, ctl, d->max_iters - 1 - ii, (float)d->opt.compact_margin,
                       d->opt.compact_margin > 0 ? (float)d->opt.compact_min_share : 0.0f, keep ? 1 : 0);
    launch_k(compact_apply_kernel, dim3(1), dim3(1024), 0, d->stream, d->d_state.p, d->d_iters.p, d->d_frame_of.p, pending, d->Bcap, s0, n,
                       d->d_perm.p, d->d_tmp3.p + (size_t)3 * s0, ctl);
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
// sizes of what it addresses before the plan is accepted (validate_class), the roles then move to device memory once.
static int build_skew_plan(lutldpc_decoder *d, int G, lutldpc_decoder::SkewPlan &plan) {
    const int I = d->max_iters, n_ops = 2 * I - 1;
    const HalfRange half[2] = {{0, (G + 1) / 2}, {(G + 1) / 2, G - (G + 1) / 2}};
    const int psc = d->psc ? 1 : 0;
    int rc;
    for (int slot = 0; slot <= n_ops; slot++) {
        std::vector<ClassParams> roles;
        lutldpc_decoder::SkewSlot sl;
        for (int hf = 0; hf < 2; hf++) {
            const int op = slot - hf;                 // B lags by one pass
            if (op < 0 || op >= n_ops) continue;
            const int ii = op / 2;
            if ((op & 1) == 0) {                      // CN(ii)
                const int check = (psc && ii > 0) ? 1 : 0;
                add_cn_roles(d, roles, half[hf], ii, check);
                if (check) { sl.state_half = hf; sl.state_ii = ii; }
            } else {                                  // VN(ii)
                add_vn_roles(d, roles, half[hf], ii, psc, (psc && !late_hard_active(d, true, nullptr)) ? 1 : 0);
            }
        }
        if ((int)roles.size() > kFusedMaxRoles) return fail(LUTLDPC_ERR_STATE, "fused launch check failed, role -1: role count");
        for (size_t r = 0; r < roles.size(); r++)
            if ((rc = validate_class(d, roles[r], "fused launch check failed, role " + std::to_string(r),
                                     {roles[r].kind ? TT_VAR : TT_CHK, false, kFusedVnDeg[d->fused_bucket_id], kFusedCnDeg[d->fused_bucket_id], "the bucket"}))) return rc;
        if ((rc = plan_items(d, roles, &sl.items, &sl.nb))) return rc;
        sl.n_roles = (int)roles.size(); sl.role_off = plan.h_roles.size();
        plan.h_roles.insert(plan.h_roles.end(), roles.begin(), roles.end());
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
