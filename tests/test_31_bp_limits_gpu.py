"""[BP] comparison decoder on the GPU (bp_decoder.hip) against references from outside the project and at its limits; the cases and
references are tests/bp_cases.py, applied to the oracle alone in tests/test_bp_exact_cpu.py.  tests/test_30_bp_gpu.py pins kernel and
oracle to each other on ordinary codes; this file pins the check pass to exact sum-product in float64, the variable pass to int64
numpy with saturation, and runs what no other test reaches: degree-2 checks, check and variable degrees up to 255, every limit
lutldpc_bp_create accepts, one handle over many batch sizes and both entries, special input values (NaN is an erasure, integer input
is clipped to +-QMAX: include/lut_ldpc_bp.h), and ber_sim's [BP] path on random codewords."""
import numpy as np
import pytest

import lut_ldpc_amd as L
import bp_cases as bc
from helpers import same
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


def _decoder(code, d=(12, 300, 7, 28)):
    return L.BPDecoder(code.nvar, code.nchk, code.dv, code.dc, code.cn_msg_idx, *d, device=0)


def _same(got, want):
    """(bits, iteration codes, output QLLRs) of two decodes."""
    for k, what in ((1, "iteration codes"), (2, "output QLLRs"), (0, "decided bits")):
        same(got[k], want[k], what)


@pytest.mark.parametrize("d", bc.STAR_SETTINGS, ids=str)
def test_check_pass_against_exact_boxplus(d):
    """The check kernel's per-edge outputs, seen through the public API on a star graph (every variable node of degree 1, one iteration,
    no exit test: LLRout - LLRin is the check-to-variable message), for three checks of each degree 2..40, 64 and 255.  A degree-2
    check returns the other input exactly; every output of a check of degree n >= 3 lies within (n - 2) * eps_op LLR units of the exact
    extrinsic boxplus of the other n - 1 quantised inputs, folded in float64 from
        a [+] b = sgn(a) sgn(b) min(|a|, |b|) + log1p(exp(-|a + b|)) - log1p(exp(-|a - b|)).
    The bound is derived, not measured: with Delta = 2^(d3-d1), one table look-up errs by at most Delta/2 (floored index, slope of
    log(1 + e^-x) at most 1/2) + 2^-(d1+1) (rounding of the entry) + log1p(exp(-d2 * Delta)) (the zero past the table's end); one integer
    boxplus has two look-ups, eps_op is twice that; exact boxplus is 1-Lipschitz in each argument and every output -- spelled-out orders
    and left/right form alike -- is an expression of exactly n - 2 boxplus operations, so the errors add."""
    graph = bc.star_graph()
    code = orc.Code(graph=graph)
    ref, dec = orc.BP(code, *d), L.BPDecoder(*graph, *d, device=0)
    assert (dec.logexp_table() == bc.table(d)).all()
    ref.set_exit_conditions(1, *bc.NO_EXIT)
    dec.set_exit_conditions(1, *bc.NO_EXIT)
    got = dec.decode_llr_batch(bc.star_llr(), want_qllr=True)
    worst = bc.check_star(d, got[2])
    print(f"star {d}: largest deviation / bound = {worst:.3f}")
    _same(got, ref.decode_llr_batch(bc.star_llr()))
    dec.close()


@pytest.mark.parametrize("d", bc.PAIR_SETTINGS, ids=str)
def test_variable_pass_against_int64_numpy_with_saturation(d):
    """Every check of degree 2: the check pass is a swap, and three iterations are mcv = mvc[partner], s = qin + bincount(mcv),
    mvc = clip(s[vn_of_edge] - mcv), LLRout = clip(s) in int64 numpy, no oracle involved.  Variable degrees 1..40, 64 and 255; in the
    two saturating settings between 10 % and 90 % of outputs and of messages clip (computed from the reference: a condition on the
    inputs)."""
    graph, _, _ = bc.pair_graph()
    want, out_share, msg_share = bc.pair_reference(d)
    assert (0.1 < out_share < 0.9 and 0.1 < msg_share < 0.9) if d in bc.PAIR_SATURATING else out_share == msg_share == 0
    dec = L.BPDecoder(*graph, *d, device=0)
    dec.set_exit_conditions(bc.PAIR_ITERS, *bc.NO_EXIT)
    bits, it, q = dec.decode_llr_batch(bc.pair_llr(), want_qllr=True)
    assert (q == want).all(), np.argwhere(q != want)[:8]
    assert (bits == (want < 0)).all() and (it == -bc.PAIR_ITERS).all()
    ref = orc.BP(orc.Code(graph=graph), *d)
    ref.set_exit_conditions(bc.PAIR_ITERS, *bc.NO_EXIT)
    _same((bits, it, q), ref.decode_llr_batch(bc.pair_llr()))
    dec.close()


@pytest.mark.parametrize("d", bc.LIMIT_SETTINGS, ids=str)
def test_every_parameter_limit_on_a_real_code(d):
    """d1, d3 = 0 and 24, d2 = 0, 1 and 2048 (the full table in LDS), d4 = 8 and 29: table, bits, LLRout and return values equal
    the oracle's in the three exit modes (bp_cases.limit_reference: at least 14 distinct return values, successes and failures,
    saturated and unsaturated outputs where d4 clips)."""
    dec = _decoder(bc.real_code(), d)
    assert (dec.logexp_table() == bc.table(d)).all()
    for mode, want in bc.limit_reference(d).items():
        dec.set_exit_conditions(bc.LIMIT_ITERS, *mode)
        _same(dec.decode_llr_batch(bc.limit_llr(), want_qllr=True), want)
    dec.close()


@pytest.mark.parametrize("d", bc.HIGH_SETTINGS, ids=["jaclog", "minsum"])
def test_high_degrees_in_a_real_decode(d):
    """Variable degrees 33, 100, 255 and check degrees 2, 33, 64, 100, 255 as guests of a (3, 6) code, ragged batch of 257."""
    code = bc.high_degree_code()
    ref, dec = orc.BP(code, *d), _decoder(code, d)
    for psc, pisc in bc.EXIT_MODES:
        ref.set_exit_conditions(bc.HIGH_ITERS, psc, pisc)
        dec.set_exit_conditions(bc.HIGH_ITERS, psc, pisc)
        want = ref.decode_llr_batch(bc.high_degree_llr())
        _same(dec.decode_llr_batch(bc.high_degree_llr(), want_qllr=True), want)
        if psc:
            assert len(set(want[1].tolist())) > 2
    dec.close()


def test_one_handle_many_shapes():
    """One handle over batches of 300, 5, 700, 256, 1 and 300 frames (the row buffers regrow once and Bpad goes 512, 256, 768, 256, 256,
    512), float and integer entry alternating, LLRout asked for or not, exit conditions changed in between."""
    d = (12, 300, 7, 28)
    code = bc.real_code()
    ref, dec = orc.BP(code, *d), _decoder(code, d)
    llr = bc.awgn(code.nvar, 700, 1.6, seed=5, rate=0.5)
    llr[3] = 9.0                                             # a noise-free frame: pisc returns 0
    steps = [(300, True, (True, True), True), (5, False, (True, False), False), (700, True, (False, False), True), (256, False, (True, True), True),
             (1, True, (True, False), False), (300, True, (True, True), True)]
    results = []
    for B, use_float, mode, want_q in steps:
        ref.set_exit_conditions(20, *mode)
        dec.set_exit_conditions(20, *mode)
        x = llr[:B]
        want = ref.decode_llr_batch(x)
        got = dec.decode_llr_batch(x, want_qllr=want_q) if use_float else dec.decode_qllr_batch(bc.to_qllr(x, d).astype(np.int32), want_qllr=want_q)
        assert (got[1] == want[1]).all() and (got[0] == want[0]).all() and (not want_q or (got[2] == want[2]).all()), B
        results.append(got)
    assert all((a == b).all() for a, b in zip(results[0], results[-1]))
    assert len(set(results[0][1].tolist())) > 2 and results[0][1][3] == 0
    dec.close()


@pytest.mark.parametrize("d", [(12, 300, 7, 28), (4, 64, 2, 8)], ids=str)
def test_special_float_inputs(d):
    """+-inf, +-0.0, all-zero frames (0 with pisc, 1 with psc alone), 30 % exact zeros, ties of the quantiser, +-QMAX / 2^d1 and its
    neighbours, 1e300, denormals: as the oracle, and through the integer entry as numpy's to_qllr.  NaN is an erasure: a frame with
    NaNs decodes as the same frame with zeros in their place, and its neighbours as without it."""
    code = bc.real_code()
    ref, dec = orc.BP(code, *d), _decoder(code, d)
    llr, zero_rows = bc.special_llr(d)
    for mode in bc.EXIT_MODES:
        ref.set_exit_conditions(10, *mode)
        dec.set_exit_conditions(10, *mode)
        got = dec.decode_llr_batch(llr, want_qllr=True)
        _same(got, ref.decode_llr_batch(llr))
        _same(dec.decode_qllr_batch(bc.to_qllr(llr, d).astype(np.int32), want_qllr=True), got)
        assert (got[1][zero_rows] == {(True, True): 0, (True, False): 1, (False, False): -10}[mode]).all() and (got[2][zero_rows] == 0).all()
    with_nan, with_zero = bc.nan_frames(llr)
    assert np.isnan(with_nan).sum() == 120
    for mode in bc.EXIT_MODES[:2]:
        ref.set_exit_conditions(10, *mode)
        dec.set_exit_conditions(10, *mode)
        got = dec.decode_llr_batch(with_nan, want_qllr=True)
        _same(got, dec.decode_llr_batch(with_zero, want_qllr=True))
        _same(got, ref.decode_llr_batch(with_nan))
        clean = np.all(with_nan == llr, axis=1)              # (NaN != NaN: the rows that hold one drop out)
        assert clean.sum() == len(llr) - 2
        ordinary = dec.decode_llr_batch(llr, want_qllr=True)
        assert all((a[clean] == b[clean]).all() for a, b in zip(got, ordinary))
    dec.close()


@pytest.mark.parametrize("d", [(12, 300, 7, 28), (4, 64, 2, 8)], ids=["d4_28", "d4_8"])
def test_integer_entry_clips_out_of_range_input(d):
    """+-(QMAX + 1), +-2^30, INT32_MAX and INT32_MIN decode exactly like np.clip(q, -QMAX, QMAX); the other frames of the batch decode
    as without them."""
    code = bc.real_code()
    ref, dec = orc.BP(code, *d), _decoder(code, d)
    q, rows = bc.out_of_range_qllr(d)
    Q = bc.qmax(d)
    assert all((q[rows] == v).any() for v in (Q + 1, -Q - 1, 2 ** 30, -2 ** 30, 2 ** 31 - 1, -2 ** 31))
    others = [r for r in range(len(q)) if r not in rows]
    assert (np.abs(q[others].astype(np.int64)) <= Q).all()
    clean = q.copy()
    clean[rows] = 0
    for mode in bc.EXIT_MODES:
        ref.set_exit_conditions(10, *mode)
        dec.set_exit_conditions(10, *mode)
        got = dec.decode_qllr_batch(q, want_qllr=True)
        _same(got, dec.decode_qllr_batch(np.clip(q, -Q, Q), want_qllr=True))
        _same(got, ref.decode_qllr_batch(q))
        without = dec.decode_qllr_batch(clean, want_qllr=True)
        assert all((a[others] == b[others]).all() for a, b in zip(got, without))
    dec.close()


def test_ber_sim_bp_section_on_random_codewords(tmp_path):
    """data/params/ber.ini.bp.example with zero_codeword = false (LDPC_BER_Sim_BP::sim_batch: host encoder, column-permuted H, bit
    errors counted against the codeword), Nframes reduced: the C++ driver and the Python driver give the five counters per SNR point
    of the oracle's frame loop on the product's graph, as test_ber_sim_bp_section_matches_oracle_frame_loop does for the zero codeword."""
    import ctypes as C
    import re
    import shutil
    from helpers import CODES, ROOT
    from lut_ldpc_amd._capi import lib, check
    from lut_ldpc_amd import ber_sim
    base = tmp_path / "base"
    (base / "codes").mkdir(parents=True)
    shutil.copy(CODES / f"{bc.REAL_CODE}.alist", base / "codes")
    txt = (ROOT / "data" / "params" / "ber.ini.bp.example").read_text()
    txt, n1 = re.subn(r"Nframes\s*=\s*2000", "Nframes  = 150", txt)
    txt, n2 = re.subn(r"zero_codeword\s*=\s*true", "zero_codeword   = false", txt)
    assert n1 == 1 and n2 == 1
    params = tmp_path / "ber.ini.bp.example"
    params.write_text(txt)
    seed, F = 2, 150
    snr = (C.c_double * 32)(); cnt = (C.c_int64 * 160)()
    n = lib.lutldpc_ber_sim_run(str(params).encode(), str(base).encode(), seed, b"", 0, 1, 1, snr, cnt, 32)
    check(min(n, 0))
    assert n == 7 and list(snr[:n]) == [0, .5, 1, 1.5, 2, 2.5, 3]
    got = np.array(cnt[:n * 5]).reshape(n, 5)
    # the oracle, frame by frame, on the product's (column-permuted) graph and the host encoder's codewords
    pcd = L.Codec(CODES / f"{bc.REAL_CODE}.alist", with_generator=True, device=-1)
    dv, dc, cn = pcd.graph()
    code = orc.Code(graph=(pcd.nvar, pcd.nchk, dv, dc, cn))
    K = pcd.nvar - pcd.nchk
    assert K == pcd.ninfo == 500
    ref = orc.BP(code, 12, 300, 7, 28)
    ref.set_exit_conditions(30, True, True)
    stop = False
    for i in range(n):
        if stop:
            assert (got[i] == 0).all()
            continue
        cw = np.stack([pcd.encode(orc.info_bits(seed, i, f, K)) for f in range(F)])
        assert cw.any()
        N0 = 10 ** (-snr[i] / 10) / 0.5
        llr, unc = orc.awgn_llr(seed, i, 0, F, code.nvar, N0, codewords=cw)
        bits, _, _ = ref.decode_llr_batch(llr)
        be = (bits[:, :K] != cw[:, :K]).sum(1)
        hit = np.flatnonzero(np.cumsum(be > 0) > 20)
        m = int(hit[0]) + 1 if hit.size else F
        want = np.array([m, m * K, (be[:m] > 0).sum(), be[:m].sum(), unc[:m].sum()])
        assert (got[i] == want).all(), (i, got[i], want)
        stop = want[3] / want[1] < 1e-7 or want[2] / want[0] < 1e-5
    assert got[0][2] == 21 and got[0][4] > 0                  # 0 dB: BP fails too, stops after Nfers + 1 frame errors
    pts, _ = ber_sim.run(params, base, seed=seed, custom_name="_py", quiet=True)
    assert (np.array([c for _, c in pts]) == got).all()
    pcd.close()
