// bp_state.hpp -- the handle of the [BP] comparison decoder and what its two units share: bp_decoder.hip (graph, decode, the
// host-input entries) and bp_frontend.hip (cell table, sampler, counters: the device front end).
#pragma once
#include "../../../include/lut_ldpc_hip.h"
#include "../../../include/lut_ldpc_bp.h"
#include "kernels_common.hpp"      // launch_k: every kernel argument segment <= 128 bytes

#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

extern "C" void lutldpc_set_last_error(const char *msg);

namespace lutldpc_bp {

inline int bp_fail(int code, const std::string &msg) { lutldpc_set_last_error(msg.c_str()); return code; }
#define BP_TRY(expr)                                                                                    \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return lutldpc_bp::bp_fail(LUTLDPC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

template <class T>
struct Buf {
    T *p = nullptr; size_t n = 0;
    hipError_t alloc(size_t c) { if (c <= n) return hipSuccess; release(); hipError_t e = hipMalloc((void **)&p, c * sizeof(T)); if (e == hipSuccess) n = c; else p = nullptr; return e; }
    hipError_t upload(const std::vector<T> &h) { hipError_t e = alloc(h.size() ? h.size() : 1); if (e != hipSuccess || h.empty()) return e; return hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice); }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    void swap(Buf &o) { std::swap(p, o.p); std::swap(n, o.n); }
};

}  // namespace lutldpc_bp

struct lutldpc_bp_decoder {
    template <class T> using Buf = lutldpc_bp::Buf<T>;
    int nvar = 0, nchk = 0, E = 0, d1 = 12, d2 = 300, d3 = 7, d4 = 28, qmax = 0;
    int max_iters = 50, psc = 1, pisc = 0, device = -1;
    std::vector<int32_t> vn_ptr, cn_ptr, cn_idx, cn_vn, table;
    hipStream_t stream = nullptr;
    Buf<int32_t> d_vn_ptr, d_cn_ptr, d_cn_idx, d_cn_vn, d_table, d_mvc, d_mcv, d_in, d_out, d_iters, d_q_in, d_q_out;
    Buf<double> d_llr;
    Buf<uint8_t> d_active, d_bits;
    Buf<uint32_t> d_fail;
    // device front end (bp_frontend.hip): the cell table with its slice index, the sent bits, the counters
    int n_cells = 0;               // 0: no table set
    Buf<uint64_t> d_thr;           // n_cells - 1 thresholds
    Buf<int32_t> d_attr;           // per cell: qllr << 1 | slicer_neg
    Buf<uint32_t> d_first;         // per slice of the unit interval: thresholds <= its lower end; one more entry = n_cells - 1
    Buf<uint8_t> d_cw;             // sent bits, frame-major
    Buf<int32_t> d_unc, d_stats;
};

namespace lutldpc_bp {
#pragma GCC visibility push(hidden)
// row buffers and per-frame state of a batch of Bpad frames
int alloc_rows(lutldpc_bp_decoder *d, int Bpad);
// bp_decode of the rows in d_in: d_out, d_iters
int decode_rows(lutldpc_bp_decoder *d, int B, int Bpad);
// rows -> frame-major on the device: bits (row value < 0) and / or the values themselves; either may be null
void store_rows(lutldpc_bp_decoder *d, const int32_t *rows, uint8_t *bits, int32_t *q, int B, int Bpad);
#pragma GCC visibility pop
}  // namespace lutldpc_bp
