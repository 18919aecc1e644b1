// llr_cells.hpp -- host half of the two LLR entries (decoder_llr.hip): the quantiser boundaries of a call turned into what the
// label kernel compares and looks up.  No device code.
//
// quant_nonlin (src/common.cpp:120-129) gives a value x the label #{leading k : x > b[k]}; for non-decreasing boundaries (anything
// else is refused by llr_cell_table; the float64 entry brings its arrays into that form first, leading_count_bounds) that is the
// plain count #{k : x > b[k]}.  The kernel never widens x.  For an input type T and a boundary
// b let b_T be the largest value of T that is <= b (-inf where b lies below -max(T), max(T) where it lies above, +inf for +inf):
// no value of T lies in (b_T, b], so for every x of type T, NaN and the infinities included, x > b exactly when x > b_T.
// Rounding down is monotone, so the b_T are non-decreasing as well.
//
// The rounded boundaries of qb_Cha and (mode 0) qb_Msg are merged, sorted and deduplicated into at most 255 thresholds u[0..n).
// The CELL of a value is #{j : x > u[j]}, one byte; inside cell c every comparison against a boundary has one outcome, so two
// 256-entry tables turn the cell into both labels: lut_cha[c] = #{k : qb_Cha_T[k] <= u[c-1]} (0 for c = 0), lut_msg likewise
// from qb_Msg_T, or map[lut_cha[c]] in mode 1.  An int8 element needs no thresholds: the byte is the cell, the tables are
// quant_nonlin((double)q * scale) for its 256 values.
#pragma once
#include "../../../include/lut_ldpc_hip.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace lutldpc {

struct LlrCells {
    int n_thr = 0;
    double thr[255];                 // values of the input type, widened; ascending, distinct
    uint8_t lut_cha[256], lut_msg[256];
};

inline size_t llr_elem_size(int dtype) {
    return dtype == LUTLDPC_LLR_F64 ? 8 : dtype == LUTLDPC_LLR_F32 ? 4 : dtype == LUTLDPC_LLR_F16 ? 2 : dtype == LUTLDPC_LLR_I8 ? 1 : 0;
}

// the largest value of a binary format (mant explicit mantissa bits, smallest normal exponent emin, largest finite value maxv)
// that is <= b; b is not NaN.  All steps are exact in double: the grid spacing at b is a power of two.
inline double round_down_to(double b, int mant, int emin, double maxv) {
    if (b > maxv) return std::isinf(b) ? b : maxv;
    if (b < -maxv) return -HUGE_VAL;
    if (b == 0.0) return b;
    int e;
    (void)std::frexp(b, &e);                                  // |b| in [2^(e-1), 2^e)
    const int q = std::max(e - 1, emin) - mant;               // spacing 2^q of the format at |b|
    return std::ldexp(std::floor(std::ldexp(b, -q)), q);
}
inline double llr_round_down(double b, int dtype) {
    if (dtype == LUTLDPC_LLR_F32) return round_down_to(b, 23, -126, 3.4028234663852886e38);
    if (dtype == LUTLDPC_LLR_F16) return round_down_to(b, 10, -14, 65504.0);
    return b;
}

inline int quant_count(double x, const double *b, int n) {
    int k = 0;
    while (k < n && x > b[k]) k++;
    return k;
}

// quant_nonlin on ANY boundary array, for the float64 entry (lutldpc_decoder_decode_llr_batch), which takes what its callers hold:
// the loop stops at the first boundary that x does not exceed, and x > max(b[0..k]) holds exactly when x exceeds every one of
// b[0..k], so the leading count over b is the plain count over its running maxima; a NaN boundary stops every x, as +inf does.
// A non-decreasing array free of NaN comes back as it is.
inline std::vector<double> leading_count_bounds(const double *b, int n) {
    std::vector<double> m(b, b + n);
    for (int k = 0; k < n; k++) {
        if (std::isnan(m[(size_t)k])) m[(size_t)k] = HUGE_VAL;
        if (k > 0 && m[(size_t)k] < m[(size_t)k - 1]) m[(size_t)k] = m[(size_t)k - 1];
    }
    return m;
}

// The checks of the entry that need no decoder and no pointer to the values, then the tables.  Returns "" or what is wrong.
inline std::string llr_cell_table(const lutldpc_llr_io &io, int Nq_Cha, int Nq_Msg0, LlrCells &C) {
    if (llr_elem_size(io.dtype) == 0) return "dtype must be LUTLDPC_LLR_F64, _F32, _F16 or _I8";
    const int mode = io.initial_message_mode;
    if (mode != 0 && mode != 1) return "initial_message_mode must be 0 (CONT) or 1 (QCHA)";
    if (Nq_Cha < 2 || Nq_Cha > 128 || Nq_Msg0 < 2 || Nq_Msg0 > 128) return "alphabet sizes must be in [2,128]";
    if (!io.qb_Cha || io.n_qb_Cha != Nq_Cha - 1) return "qb_Cha must hold Nq_Cha-1 boundaries";
    if (mode == 0 && (!io.qb_Msg || io.n_qb_Msg != Nq_Msg0 - 1)) return "mode 0 (CONT): qb_Msg must hold Nq_Msg[0]-1 boundaries";
    if (mode == 0 && io.cha2msg_map) return "mode 0 (CONT): cha2msg_map must be NULL";
    if (mode == 1 && !io.cha2msg_map) return "mode 1 (QCHA) needs cha2msg_map";
    const int n_cha = Nq_Cha - 1, n_msg = mode == 0 ? Nq_Msg0 - 1 : 0;
    for (int k = 0; k < n_cha; k++)
        if (std::isnan(io.qb_Cha[k]) || (k > 0 && io.qb_Cha[k] < io.qb_Cha[k - 1])) return "qb_Cha must be non-decreasing and free of NaN";
    for (int k = 0; k < n_msg; k++)
        if (std::isnan(io.qb_Msg[k]) || (k > 0 && io.qb_Msg[k] < io.qb_Msg[k - 1])) return "qb_Msg must be non-decreasing and free of NaN";
    for (int i = 0; mode == 1 && i < Nq_Cha; i++)
        if (io.cha2msg_map[i] < 0 || io.cha2msg_map[i] >= Nq_Msg0) return "cha2msg_map entry outside [0, Nq_Msg[0])";
    if (io.dtype == LUTLDPC_LLR_I8 && !(std::isfinite(io.scale) && io.scale > 0.0)) return "LUTLDPC_LLR_I8 needs a finite scale > 0";

    C.n_thr = 0;
    if (io.dtype == LUTLDPC_LLR_I8) {
        for (int q = -128; q < 128; q++) {
            const double x = (double)q * io.scale;
            const int a = quant_count(x, io.qb_Cha, n_cha);
            C.lut_cha[(uint8_t)q] = (uint8_t)a;
            C.lut_msg[(uint8_t)q] = (uint8_t)(mode == 0 ? quant_count(x, io.qb_Msg, n_msg) : io.cha2msg_map[a]);
        }
        return "";
    }
    std::vector<double> cha(io.qb_Cha, io.qb_Cha + n_cha), msg(io.qb_Msg, io.qb_Msg + n_msg), u;
    for (double &b : cha) b = llr_round_down(b, io.dtype);
    for (double &b : msg) b = llr_round_down(b, io.dtype);
    u = cha;
    u.insert(u.end(), msg.begin(), msg.end());
    std::sort(u.begin(), u.end());
    u.erase(std::unique(u.begin(), u.end()), u.end());      // (-0.0 == 0.0: one threshold)
    C.n_thr = (int)u.size();                                // <= 127 + 127
    std::copy(u.begin(), u.end(), C.thr);
    for (int c = 0; c < 256; c++) {
        int a = 0, m = 0;
        if (c > 0) {
            const double top = u[(size_t)std::min(c, C.n_thr) - 1];
            while (a < n_cha && cha[(size_t)a] <= top) a++;
            while (m < n_msg && msg[(size_t)m] <= top) m++;
        }
        C.lut_cha[c] = (uint8_t)a;
        C.lut_msg[c] = (uint8_t)(mode == 0 ? m : io.cha2msg_map[a]);
    }
    return "";
}

}  // namespace lutldpc
