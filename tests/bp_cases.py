"""The cases of the [BP] comparison decoder's tests against references from outside the project, shared by
tests/test_31_bp_limits_gpu.py (decodes them on the GPU) and tests/test_bp_exact_cpu.py (applies the same references to the oracle,
so the references themselves are checked where there is no GPU).  Product (bp_decoder.hip) and oracle (oracle/or_bp.c) were written
from the same paragraph of include/lut_ldpc_bp.h and tests/test_30_bp_gpu.py pins them to each other only: a mistake shared by both
(the signs of the jac-log correction, the table formula) would pass there.  Here the check pass is compared with exact sum-product
in float64 (section 1) and the variable pass with plain int64 numpy (section 2); the other sections take the kernels to the limits
lutldpc_bp_create accepts and through inputs the header had left open.

Section 1, the bound.  With Delta = 2^(d3-d1) LLR units per table step, one look-up logexp(x) errs against log(1 + exp(-x / 2^d1)) by
at most Delta/2 (the index is floored and the slope of log(1 + e^-x) is at most 1/2) + 2^-(d1+1) (rounding of the entry) +
log1p(exp(-d2 * Delta)) (the zero past the table's end).  One integer boxplus holds two look-ups and nothing else inexact (the
sign-min term and the sums are exact integers), so it errs by eps_op = twice that.  Exact boxplus is 1-Lipschitz in each argument,
and every output of a check of degree n -- in the spelled-out orders of degrees 3..6 and in the left/right form -- is an expression of
exactly n - 2 boxplus operations on n - 1 inputs, so the errors add to at most (n - 2) * eps_op.  Exact boxplus is associative: the
reference may fold in any order."""
from __future__ import annotations

import functools

import numpy as np

from helpers import CODES, write_degree_alist
from oracle import oracle as orc

NO_EXIT = (False, False)                                    # (psc, pisc): every frame runs max_iters iterations
EXIT_MODES = [(True, True), (True, False), (False, False)]
REAL_CODE = "rate0.50_dv03_dc06_N1000"


def qmax(d):
    return 2 ** (d[3] - 1) - 1


def to_qllr(llr, d):
    """include/lut_ldpc_bp.h in numpy: clip(floor(0.5 + 2^d1 * l), +-QMAX), NaN -> 0; int64."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.floor(0.5 + np.asarray(llr, np.float64) * 2.0 ** d[0])
    t = np.where(np.isnan(t), 0.0, np.clip(t, -qmax(d), qmax(d)))
    return t.astype(np.int64)


def table(d):
    """T[i] = to_qllr(log(1 + exp(-i * 2^(d3-d1)))), i < d2."""
    return to_qllr(np.log1p(np.exp(-np.arange(d[1]) * 2.0 ** (d[2] - d[0]))), d).astype(np.int32)


def awgn(nvar, B, snr_db, seed, rate):
    """All-zero codeword over BPSK / AWGN, LLR = 4x / N0."""
    rng = np.random.default_rng(seed)
    N0 = 10 ** (-snr_db / 10) / rate
    return 4 * (1.0 + rng.normal(0.0, np.sqrt(N0 / 2), (B, nvar))) / N0


def mixed_scale_llr(B, N, scales, seed):
    """Normal samples scaled per entry by one of `scales`: a wide range of magnitudes in every frame."""
    rng = np.random.default_rng(seed)
    llr = rng.normal(0.0, 1.0, (B, N)) * rng.choice(scales, size=(B, N))
    llr.setflags(write=False)
    return llr


def real_code():
    return orc.Code(CODES / f"{REAL_CODE}.alist")


# ---- section 1: the check pass alone.  A star graph: every variable node has degree 1, so with one iteration and no exit test
#      LLRout[v] - LLRin[v] is the check-to-variable message on v's only edge
STAR_SETTINGS = [(12, 300, 7, 28), (12, 2048, 4, 28), (8, 64, 4, 16)]
STAR_DEGREES = [n for n in list(range(2, 41)) + [64, 255] for _ in range(3)]
STAR_B, STAR_SCALES, STAR_SEED = 64, (0.3, 2.0, 6.0), 31


def star_graph():
    """(nvar, nchk, dv, dc, cn_msg_idx): three checks of every degree in STAR_DEGREES; edge e belongs to variable e, and the edges of
    a check are consecutive and ascend."""
    dc = np.array(STAR_DEGREES, np.int32)
    E = int(dc.sum())
    return E, len(dc), np.ones(E, np.int32), dc, np.arange(E, dtype=np.int32)


def star_llr():
    return mixed_scale_llr(STAR_B, int(np.sum(STAR_DEGREES)), STAR_SCALES, STAR_SEED)


def eps_op(d):
    """Largest error of one integer boxplus against exact boxplus, in LLR units (module docstring)."""
    delta = 2.0 ** (d[2] - d[0])
    return 2 * (delta / 2 + 2.0 ** -(d[0] + 1) + np.log1p(np.exp(-d[1] * delta)))


def boxplus_exact(a, b):
    """a [+] b in float64: exact, stable at any magnitude (atanh(prod tanh) loses the large ones), associative."""
    return np.sign(a) * np.sign(b) * np.minimum(np.abs(a), np.abs(b)) + np.log1p(np.exp(-np.abs(a + b))) - np.log1p(np.exp(-np.abs(a - b)))


def extrinsic_exact(x):
    """x [..., n]: for every i the exact boxplus of the other n - 1 entries (prefix and suffix folds)."""
    n = x.shape[-1]
    left, right = np.empty_like(x), np.empty_like(x)       # left[i] = x[0] [+] .. [+] x[i], right[i] = x[i] [+] .. [+] x[n-1]
    left[..., 0], right[..., n - 1] = x[..., 0], x[..., n - 1]
    for i in range(1, n):
        left[..., i] = boxplus_exact(left[..., i - 1], x[..., i])
        right[..., n - 1 - i] = boxplus_exact(right[..., n - i], x[..., n - 1 - i])
    out = np.empty_like(x)
    out[..., 0], out[..., n - 1] = right[..., 1], left[..., n - 2]
    for i in range(1, n - 1):
        out[..., i] = boxplus_exact(left[..., i - 1], right[..., i + 1])
    return out


@functools.lru_cache(maxsize=None)
def star_reference(d):
    """(qin [B, E] int64, exact check-to-variable messages [B, E] in LLR units) for the quantised inputs of setting d: input
    quantisation is not part of the error."""
    qin = to_qllr(star_llr(), d)
    x = qin / 2.0 ** d[0]
    want = np.empty_like(x)
    e = 0
    for n in STAR_DEGREES:
        want[:, e:e + n] = x[:, e:e + n][:, ::-1] if n == 2 else extrinsic_exact(x[:, e:e + n])
        e += n
    qin.setflags(write=False)
    want.setflags(write=False)
    return qin, want


def check_star(d, out_qllr):
    """The assertions of section 1 on the LLRout of one iteration without exit test.  Returns the largest deviation over bound."""
    qin, want = star_reference(d)
    assert np.abs(qin).max() < qmax(d) // 2                                  # nothing clips: LLRout - LLRin is the message
    mcv = np.asarray(out_qllr, np.int64) - qin
    worst, e = 0.0, 0
    for n in STAR_DEGREES:
        got = mcv[:, e:e + n]
        if n == 2:
            assert (got == qin[:, e:e + n][:, ::-1]).all(), "degree-2 check: each edge must return the other input exactly"
        else:
            dev = np.abs(got / 2.0 ** d[0] - want[:, e:e + n]).max()
            bound = (n - 2) * eps_op(d)
            assert dev <= bound, (d, n, e, dev, bound)
            worst = max(worst, dev / bound)
        e += n
    return worst


# ---- section 2: the variable pass alone.  Every check has degree 2, so the check pass is a swap and numpy states the decoder in int64
PAIR_SETTINGS = [(12, 300, 7, 28), (4, 64, 2, 8), (24, 2048, 24, 29)]       # nothing clips; QMAX = 127; QMAX = 2^28 - 1
PAIR_SATURATING = PAIR_SETTINGS[1:]
PAIR_VDEG = [n for n in range(1, 41) for _ in range(3)] + [64, 64, 255, 255] + [3] * 600
PAIR_B, PAIR_ITERS, PAIR_SCALES, PAIR_SEED = 32, 3, (0.2, 1.0, 4.0), 7


@functools.lru_cache(maxsize=None)
def pair_graph():
    """(nvar, nchk, dv, dc, cn_msg_idx), partner [E], vn_of_edge [E]: the sockets of the variable nodes paired at random; a check
    that would join a node to itself or repeat another check's pair of nodes swaps partners with a random other check."""
    rng = np.random.default_rng(PAIR_SEED)
    dv = np.array(PAIR_VDEG, np.int32)
    E = int(dv.sum())
    vn = np.repeat(np.arange(len(dv)), dv)
    pairs = rng.permutation(E).reshape(-1, 2)
    for _ in range(1000):
        a, b = np.minimum(vn[pairs[:, 0]], vn[pairs[:, 1]]), np.maximum(vn[pairs[:, 0]], vn[pairs[:, 1]])
        key = a.astype(np.int64) * len(dv) + b
        _, first, count = np.unique(key, return_index=True, return_counts=True)
        bad = np.ones(len(pairs), bool)
        bad[first] = False                                                  # repeated pairs: all but the first
        bad |= a == b
        if not bad.any():
            break
        for c in np.flatnonzero(bad):
            o = int(rng.integers(len(pairs)))
            pairs[c, 1], pairs[o, 1] = pairs[o, 1], pairs[c, 1]
    else:
        raise AssertionError("pair graph not repaired")
    pairs = np.sort(pairs, axis=1)                                          # edge ids within a check ascend
    partner = np.empty(E, np.int64)
    partner[pairs[:, 0]], partner[pairs[:, 1]] = pairs[:, 1], pairs[:, 0]
    M = len(pairs)
    return (len(dv), M, dv, np.full(M, 2, np.int32), pairs.reshape(-1).astype(np.int32)), partner, vn


def pair_llr():
    return mixed_scale_llr(PAIR_B, len(PAIR_VDEG), PAIR_SCALES, PAIR_SEED)


@functools.lru_cache(maxsize=None)
def pair_reference(d):
    """PAIR_ITERS iterations in int64: (LLRout [B, N], share of outputs that clip, share of variable-to-check messages that clip)."""
    (N, M, dv, _, _), partner, vn = pair_graph()
    Q = qmax(d)
    qin = to_qllr(pair_llr(), d)
    ptr = np.concatenate([[0], np.cumsum(dv)])[:-1]
    mvc = qin[:, vn]
    clipped_msgs = total_msgs = 0
    for _ in range(PAIR_ITERS):
        mcv = mvc[:, partner]
        s = qin + np.add.reduceat(mcv, ptr, axis=1)
        ext = s[:, vn] - mcv
        clipped_msgs, total_msgs = clipped_msgs + int((np.abs(ext) > Q).sum()), total_msgs + ext.size
        mvc = np.clip(ext, -Q, Q)
    out = np.clip(s, -Q, Q)
    out.setflags(write=False)
    return out, float((np.abs(s) > Q).mean()), clipped_msgs / total_msgs


# ---- section 3: every limit lutldpc_bp_create accepts, on a real code
LIMIT_SETTINGS = [(4, 64, 2, 8), (0, 1, 0, 8), (0, 0, 0, 8), (24, 2048, 24, 29), (24, 2048, 20, 29), (12, 2048, 4, 28), (12, 1, 7, 28)]
LIMIT_SATURATING = [LIMIT_SETTINGS[0], LIMIT_SETTINGS[3], LIMIT_SETTINGS[4]]
LIMIT_REFUSED = [(25, 300, 7, 28), (12, 2049, 7, 28), (12, 300, 25, 28), (12, 300, 7, 7), (12, 300, 7, 30)]       # one step past each limit
LIMIT_B, LIMIT_SNR, LIMIT_ITERS, LIMIT_SEED = 70, 2.0, 25, 3


@functools.lru_cache(maxsize=None)
def limit_llr():
    llr = awgn(1000, LIMIT_B, LIMIT_SNR, seed=LIMIT_SEED, rate=0.5)
    llr.setflags(write=False)
    return llr


@functools.lru_cache(maxsize=None)
def limit_reference(d):
    """The oracle's (bits, return values, LLRout) per exit mode, and that the case is no degenerate one: with early exit at least 14
    distinct return values, successes and failures; in the saturating settings clipped and unclipped outputs (share of |LLRout| = QMAX
    with early exit between 10 % and 95 %)."""
    ref = orc.BP(real_code(), *d)
    assert (ref.table() == table(d)).all()
    out = {}
    for psc, pisc in EXIT_MODES:
        ref.set_exit_conditions(LIMIT_ITERS, psc, pisc)
        out[(psc, pisc)] = ref.decode_llr_batch(limit_llr())
    it = out[(True, False)][1]
    assert len(set(it.tolist())) >= 14 and (it > 0).any() and (it < 0).any(), (d, sorted(set(it.tolist())))
    if d in LIMIT_SATURATING:
        share = float((np.abs(out[(True, False)][2]) == qmax(d)).mean())
        assert 0.1 < share < 0.95, (d, share)
    return out


# ---- section 4: high degrees in a real decode.  Degree-3 variable nodes and degree-6 checks carry the code; the guests are a few
#      nodes each, no class size a multiple of 4
HIGH_VDEG = {3: 670, 33: 3, 100: 3, 255: 2}
HIGH_CDEG = {2: 6, 6: 301, 33: 3, 64: 3, 100: 3, 255: 2}
HIGH_B, HIGH_ITERS, HIGH_SNR, HIGH_SEED = 257, 10, 5.5, 4      # the high-degree checks carry little: 5.5 dB for a mix of exits
HIGH_SETTINGS = [(12, 300, 7, 28), (12, 0, 7, 28)]                           # jac-log, min-sum


@functools.lru_cache(maxsize=None)
def high_degree_code():
    import tempfile
    with tempfile.TemporaryDirectory(prefix="bp_cases_") as tmp:
        write_degree_alist(f"{tmp}/high.alist", HIGH_VDEG, HIGH_CDEG, seed=HIGH_SEED)
        code = orc.Code(f"{tmp}/high.alist")
    assert sorted(set(code.dv.tolist())) == sorted(HIGH_VDEG) and sorted(set(code.dc.tolist())) == sorted(HIGH_CDEG)
    return code


@functools.lru_cache(maxsize=None)
def high_degree_llr():
    code = high_degree_code()
    llr = awgn(code.nvar, HIGH_B, HIGH_SNR, seed=HIGH_SEED, rate=1.0 - code.nchk / code.nvar)
    llr.setflags(write=False)
    return llr


# ---- section 6: special input values
def special_llr(d, seed=6):
    """(llr [B, N], rows that are all zero): ordinary frames of the real code at 2 dB with special values scattered over a few of them.
    Row 0 stays ordinary, rows 1..: +-inf, +-0.0, all zero (two rows), 30 % exact zeros, ties of the quantiser, +-QMAX / 2^d1 and one
    step inside and outside it, 1e300, denormals."""
    rng = np.random.default_rng(seed)
    llr = awgn(1000, 12, 2.0, seed=seed, rate=0.5)
    N, s, Q = llr.shape[1], 2.0 ** d[0], qmax(d)

    def scatter(row, values, n=40):
        pos = rng.choice(N, size=n, replace=False)
        llr[row, pos] = np.resize(np.asarray(values, np.float64), n)

    scatter(1, [np.inf, -np.inf])
    scatter(2, [0.0, -0.0])
    llr[3] = 0.0
    llr[4] = -0.0
    llr[5, rng.random(N) < 0.3] = 0.0
    scatter(6, [(k + 0.5) / s for k in (0, 1, 2, 7, 100, -1, -2, -3, -8, -101)])
    scatter(7, [sg * (Q + k) / s for sg in (1, -1) for k in (-1, 0, 1)] + [sg * (Q + k + 0.5) / s for sg in (1, -1) for k in (-2, -1, 0)])
    scatter(8, [1e300, -1e300])
    scatter(9, [5e-324, -5e-324, 2.2e-308, -2.2e-308, 1e-310])
    return llr, [3, 4]


def nan_frames(llr, rows=(1, 10), seed=9):
    """(llr with NaNs planted in `rows`, the same with zeros in their place)."""
    rng = np.random.default_rng(seed)
    with_nan, with_zero = llr.copy(), llr.copy()
    for r in rows:
        pos = rng.choice(llr.shape[1], size=60, replace=False)
        with_nan[r, pos], with_zero[r, pos] = np.nan, 0.0
    return with_nan, with_zero


def out_of_range_qllr(d, seed=8):
    """(q [B, N] int32 with values beyond +-QMAX planted in rows 1 and 3, the rows that hold them): +-(QMAX+1), +-2^30, INT32_MAX, INT32_MIN."""
    rng = np.random.default_rng(seed)
    q = to_qllr(awgn(1000, 6, 2.0, seed=seed, rate=0.5), d).astype(np.int32)
    Q = qmax(d)
    vals = np.array([Q + 1, -(Q + 1), 2 ** 30, -2 ** 30, 2 ** 31 - 1, -2 ** 31], np.int64).astype(np.int32)
    rows = [1, 3]
    for r in rows:
        pos = rng.choice(q.shape[1], size=48, replace=False)
        q[r, pos] = np.resize(vals, 48)
    return q, rows
