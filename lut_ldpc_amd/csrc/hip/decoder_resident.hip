// decoder_resident.hip -- the LDS-resident decoder (jit_resident.hpp): eligibility, geometry, kernel generation, launch.
#include "decoder_state.hpp"

#pragma GCC visibility push(hidden)

constexpr int kLdsPerCu = 160 * 1024, kResidentCus = 256;

ResidentSpec resident_spec(const lutldpc_decoder *d, int S, int NT) {
    ResidentSpec R;
    R.pack = d->pack; R.N = d->nvar; R.E = d->E; R.S = S; R.NT = NT; R.I = d->max_iters_created; R.nq_cha = d->Nq_Cha; R.min_lut = d->min_lut;
    R.nq_msg = d->Nq_Msg; R.iter_set = d->iter_set; R.U = d->opt.resident_U; R.xcd = d->opt.resident_xcd; R.waves_eu = d->opt.resident_waves_eu;
    {   // wave-reduced exit-test flags cost registers in the item bodies: +7 % on (3,6) N=10000 as shipped, but with the wide trees of
        // N=500 (degree 17: 168 registers, one wave per SIMD less) 13.5 -> 10.2 M codewords/s -- only where the trees are small
        int max_vn = 0;
        for (auto &c : d->vclass) max_vn = std::max(max_vn, c.deg);
        R.flag_reduce = d->opt.resident_flag_reduce >= 0 ? d->opt.resident_flag_reduce : (max_vn <= 8 ? 1 : 0);
        // check items keep their LDS addresses in registers when that is few registers and the trees leave room for them
        int cn_regs = 0, max_cn = 0;
        for (auto &c : d->cclass) { cn_regs += (int)((S * (long long)c.nodes.size() + NT - 1) / NT + 1) * c.deg; max_cn = std::max(max_cn, c.deg); }
        // (... or the wide trees have cost the occupancy already: N=500 runs two waves per SIMD with 159 registers, +3 % with them;
        // (6,32) N=2048 would fall from three workgroups per compute unit to two: 25.6 -> 23.5 M, off)
        R.cn_persistent = d->opt.resident_cn_persistent >= 0 ? d->opt.resident_cn_persistent
                          : (d->min_lut && max_cn <= 16 && ((max_vn <= 4 && cn_regs <= 40) || (max_vn > 12 && cn_regs <= 96)) ? 1 : 0);      // (measured: (3,6) N=10000 1.82 -> 1.92 M codewords/s fixed work, 3.65 -> 3.93 M as shipped)
    }
    for (auto &c : d->vclass) R.vcls.push_back({c.deg, (int)c.nodes.size(), c.tidx_off, 0});
    for (auto &c : d->cclass) R.ccls.push_back({c.deg, (int)c.nodes.size(), c.tidx_off, c.tnidx_off});
    // the trees as they are; checks over full labels where that form exists (one instruction per look-up)
    const size_t ns = d->tree_plans[TT_VAR].size();
    R.var.assign(ns, {}); R.dec.assign(ns, {}); R.chk.assign(ns, {});
    for (size_t s = 0; s < ns; s++) {
        for (auto &c : d->tree_set(TT_VAR, (int)s)->cls) R.var[s].push_back(&c.base);
        for (auto &c : d->tree_set(TT_DEC, (int)s)->cls) R.dec[s].push_back(&c.base);
        for (size_t c = 0; c < d->tree_set(TT_CHK, (int)s)->cls.size(); c++) R.chk[s].push_back(d->chk_form((int)s, (int)c));
    }
    return R;
}

// can this code be decoded out of LDS at all (one set per workgroup)?
bool resident_eligible(const lutldpc_decoder *d) {
    if (!d->opt.use_resident || !d->opt.use_jit || !d->opt.use_fast || d->device < 0) return false;
    if (d->min_lut) for (int nq : d->Nq_Msg) if (!is_pow2(nq / 2)) return false;
    for (auto &c : d->cclass) if (c.deg < 2 || c.deg > 64) return false;
    // wide CHKTREE checks (a 31-leaf tree: 184 look-ups per frame and check, inputs / outputs / edge ids of 32 edges in registers) run
    // faster through the streaming pass kernels: (6,32) N=2048 with min_lut = false 7.4 M codewords/s against 5.6 M out of LDS
    if (!d->min_lut && d->opt.use_resident < 2) for (auto &c : d->cclass) if (c.deg > 16) return false;      // (LUTLDPC_RESIDENT=2 forces it)
    for (auto &c : d->vclass) if (c.deg > 24) return false;
    if (d->vclass.size() > 12 || d->cclass.size() > 12) return false;
    const ResidentSpec R = resident_spec(d, 1, 1024);
    return resident_lds_bytes(R) <= kLdsPerCu - 2048;
}

// Sets per workgroup (S) and workgroup size (NT) for a batch of G frame groups.  Rules read off tools/resident_probe.py sweeps on
// MI355X (profiles/r03_resident_geometry_sweep.txt):
//   * two or three workgroups per compute unit beat one large one -- their check and variable phases interleave on the vector
//     ALUs and the LDS: (6,32) N=2048 23.6 M codewords/s at S = 1 / 512 threads (three workgroups of 51 KB) against 19.3 M at
//     S = 2 / 1024 -- so S is the largest value that leaves room for two workgroups (<= 78 KB of LDS each) ...
//   * ... and gives a thread about eight variable-node items: every pass of a workgroup costs two barriers and a table staging
//     whatever its size, and the items of a heavy degree class spread evenly only when there are many (N=500: 13.3 M at
//     S = 8 / 512, 9.4 M at S = 2 / 256, 6.2 M at S = 2 / 1024);
//   * a code that fills the LDS with a single set ((3,6) N=10000: 120 KB) runs one workgroup of 1024 threads;
//   * a batch too small to give every compute unit its workgroups takes a smaller S.
// LUTLDPC_RESIDENT_S / LUTLDPC_RESIDENT_NT override.
bool resident_pick(const lutldpc_decoder *d, int G, int &S_out, int &NT_out, int &lds_out) {
    const long long sets = 64ll * G;
    auto lds_of = [&](int S, int NT) { return resident_lds_bytes(resident_spec(d, S, NT)); };
    auto items_of = [&](int S, int NT) { return (int)((S * (long long)d->nvar + NT - 1) / NT) + (int)d->vclass.size(); };
    const int budget = kLdsPerCu - 2048;
    if (lds_of(1, 512) > budget) return false;
    int S = 1, NT = 512;
    if (d->opt.resident_force_S || d->opt.resident_force_NT) {
        S = d->opt.resident_force_S ? d->opt.resident_force_S : 1;
        NT = d->opt.resident_force_NT ? d->opt.resident_force_NT : 512;
    } else if (lds_of(1, 512) > 78 * 1024) {
        NT = 1024;                                              // one workgroup per compute unit: all the waves it can hold
    } else {
        while (S < 64 && lds_of(S + 1, NT) <= 78 * 1024 && (S + 1) * (long long)d->nvar <= 8ll * NT + NT / 2) S++;
        while (S > 1 && (sets + S - 1) / S < (long long)kResidentCus) S--;        // small batch: at least one workgroup per compute unit
    }
    while (S > 1 && (lds_of(S, NT) > budget || items_of(S, NT) > 46)) S--;
    if (lds_of(S, NT) > budget || items_of(S, NT) > 46) {
        if (NT < 1024 && items_of(S, 1024) <= 46 && lds_of(S, 1024) <= budget) NT = 1024; else return false;
    }
    S_out = S; NT_out = NT; lds_out = lds_of(S, NT);
    return true;
}

int resident_plan_for(lutldpc_decoder *d, int G, lutldpc_decoder::ResidentPlan **out) {
    auto it = d->resident_plans.find(G);
    if (it == d->resident_plans.end()) {
        lutldpc_decoder::ResidentPlan pl;
        if (!resident_pick(d, G, pl.S, pl.NT, pl.lds)) return fail(LUTLDPC_ERR_STATE, "resident decoder: no configuration fits");
        // equal (S, NT) of another batch size: the same kernel
        for (auto &kv : d->resident_plans) if (kv.second.S == pl.S && kv.second.NT == pl.NT) pl.k = kv.second.k;
        if (!pl.k) {
            std::string src, err, log;
            if (!jit_resident_source(resident_spec(d, pl.S, pl.NT), src, err)) return fail(LUTLDPC_ERR_UNSUPPORTED, "resident decoder: " + err);
            JitKernel *k = jit_get(d->device, src, log);
            if (!k) return fail(LUTLDPC_ERR_STATE, "generated-kernel registry full");
            if (!log.empty()) { d->resident_log = log; return fail(LUTLDPC_ERR_HIP, "resident decoder: hiprtc / module load failed: " + log.substr(0, 2000)); }
            if (!k->ok()) return fail(LUTLDPC_ERR_HIP, "resident decoder: kernel unavailable (earlier compile failure)");
            pl.k = k;
        }
        it = d->resident_plans.emplace(G, pl).first;
    }
    *out = &it->second;
    return LUTLDPC_OK;
}

int launch_resident(lutldpc_decoder *d, int G, int B, const FrameMajorIO *fm) {
    lutldpc_decoder::ResidentPlan *pl = nullptr;
    if (int rc = resident_plan_for(d, G, &pl)) return rc;
    Timed t(d, LUTLDPC_K_RESIDENT);
    ResidentArgs A{};
    A.cha = d->d_cha_t.p; A.msg0 = d->d_msg0_t.p; A.hard = d->d_hard.p; A.state = d->d_state.p; A.iters = d->d_iters.p;
    A.tables = d->d_tables.p; A.idx = d->d_fast_idx.p; A.n_sets = 64 * G; A.max_iters = d->max_iters; A.psc = d->psc; A.pisc = d->pisc;
    A.B = B; A.lim_cha = d->Nq_Cha - 1; A.lim_msg = d->Nq_Msg[0] - 1;
    if (fm) { A.fm_cha = fm->cha; A.fm_msg0 = fm->msg0; A.fm_bits = fm->bits; }
    void *args[] = {&A};
    const unsigned blocks = (unsigned)((64 * G + pl->S - 1) / pl->S);
    HIP_TRY(hipModuleLaunchKernel(pl->k->fn, blocks, 1, 1, (unsigned)pl->NT, 1, 1, 0, d->stream, args, nullptr));
    LAUNCH_CHECK();
    return LUTLDPC_OK;
}

#pragma GCC visibility pop
