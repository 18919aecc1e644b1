"""The [BP] decoder's device front end on the GPU (include/lut_ldpc_bp.h: lutldpc_bp_set_cells, lutldpc_bp_sample_qllr,
lutldpc_bp_sim_batch, BP.front_end = device in ber_sim) against references from outside the code under test
(tests/bp_frontend_cases.py): the numpy Philox sampler with np.searchsorted as the cell, the oracle's BP.decode_qllr_batch, plain
numpy counting.  Everything is integer and has to be equal, sample for sample and frame for frame."""
import ctypes as C
import re
import shutil

import numpy as np
import pytest

import bp_frontend_cases as BC
import lut_ldpc_amd as L
from helpers import CODES, ROOT, same
from lut_ldpc_amd import _capi
from lut_ldpc_amd._capi import lib, check, ERR_ARG, ERR_STATE
from lut_ldpc_amd.bp import awgn_cells
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

_handles = {}


def handle(code):
    """One decoder per graph for the whole module: the cases replace its table and change its batch size over and over."""
    if code not in _handles:
        g = BC.sim_code(code[4:])[0] if code.startswith("sim-") else BC.graph(code)
        _handles[code] = L.BPDecoder(g.nvar, g.nchk, g.dv, g.dc, g.cn_msg_idx, *BC.D, device=0)
    return _handles[code]


@pytest.mark.parametrize("case", BC.SAMPLER_CASES, ids=BC.case_id)
def test_sampler_equals_numpy_for_every_sample(case):
    code, table, B, f0, seed, stream, _ = case
    cells, u, N, B, cw = BC.sampler_case(case)
    dec = handle(code)
    dec.set_cells(cells)
    want_q, want_unc = BC.sample(cells, seed, stream, f0, B, N, cw, u=u)
    got_q, got_unc = dec.sample_qllr(seed, stream, f0, B, cw)
    same(got_q, want_q, "qllr", u)
    same(got_unc, want_unc, "uncoded errors")


@pytest.mark.parametrize("nonzero", [False, True], ids=["zero", "codewords"])
@pytest.mark.parametrize("name", sorted(BC.SIM_CASES))
def test_sim_batch_equals_sampler_oracle_and_counts(name, nonzero):
    _, _, iters, K = BC.SIM_CASES[name]
    g, cw, _ = BC.sim_code(name)
    cw = cw if nonzero else None
    dec = handle("sim-" + name)
    dec.set_cells(BC.awgn_table(BC.sim_n0(name)))
    args = (BC.SIM_SEED, BC.SIM_STREAM, 0, BC.SIM_B)
    for psc, pisc in BC.EXIT_MODES:
        ref = BC.sim_reference(name, psc, pisc, nonzero)
        dec.set_exit_conditions(iters, psc, pisc)
        stats, q, bits = dec.sim_batch(*args, K, cw, want_qllr=True, want_bits=True)
        same(q, ref["q"], "qllr_out")
        same(stats[:, 0], ref["iters"], "bp_decode return value")
        same(bits, ref["bits"], "bits_out")
        same(stats, ref["stats"], "frame_stats")
        # the entries agree with each other: sample_qllr on the same arguments, then decode_qllr_batch on the same handle
        q2, unc2 = dec.sample_qllr(*args, cw)
        same(q2, q, "sample_qllr against qllr_out")
        bits2, it2 = dec.decode_qllr_batch(q2)
        same(BC.count(bits2, it2, unc2, K, cw), stats, "sample_qllr + decode_qllr_batch against sim_batch")
        same(dec.sim_batch(*args, K, cw), stats, "frame_stats alone")
        for k in (0, g.nvar):                                                    # K_info at its limits
            same(dec.sim_batch(*args, k, cw), BC.count(ref["bits"], ref["iters"], ref["unc"], k, cw), f"K_info = {k}")


@pytest.mark.parametrize("zero_codeword", [True, False], ids=["zero", "codewords"])
def test_paired_noise_with_the_lut_front_end(zero_codeword):
    """Frame f of a [BP] run sees the received values of frame f of a [LUT] run with the same seed and stream: the slicer errors per
    frame are equal, with the all-zero codeword and with the codewords the LUT run sends."""
    from helpers import product_codec
    cd = product_codec("n500_q4_i8", device=0) if zero_codeword else None
    if cd is None:
        cd = L.Codec(CODES / f"{BC.N500}.alist", with_generator=True, device=0)
        cd.design_luts(sigma2=0.88 ** 2, max_iters=8, nq_cha=16, nq_msg=16)
    snr, seed, stream, f0, B = 1.6, 2 ** 40 + 5, 3, 2 ** 32 - 100, 600
    lut = cd.sim_batch(snr, seed, stream, f0, B, zero_codeword=zero_codeword)
    cw = None if zero_codeword else cd.encode_random(seed, stream, f0, B)
    dv, dc, cn = cd.graph()
    dec = L.BPDecoder(cd.nvar, cd.nchk, dv, dc, cn, *BC.D, device=0)
    cells = awgn_cells(10 ** (-snr / 10) / cd.rate)
    dec.set_cells(cells)
    dec.set_exit_conditions(8, True, True)
    bp = dec.sim_batch(seed, stream, f0, B, cd.ninfo, cw)
    assert lut[:, 3].min() < lut[:, 3].max() and lut[:, 3].sum() > 20 * B
    same(bp[:, 3], lut[:, 3], "uncoded errors per frame, [BP] against [LUT]")
    same(bp[:, 3], BC.sample(cells, seed, stream, f0, B, cd.nvar, cw)[1], "uncoded errors per frame against numpy")
    dec.close()


def _run_ber_sim(tmp_path, front_end, nframes=150, zero_codeword=True):
    base = tmp_path / f"base_{front_end}_{int(zero_codeword)}"
    (base / "codes").mkdir(parents=True)
    shutil.copy(CODES / "rate0.50_dv03_dc06_N1000.alist", base / "codes")
    txt = (ROOT / "data" / "params" / "ber.ini.bp.example").read_text()
    txt = re.sub(r"Nframes\s*=\s*2000", f"Nframes  = {nframes}", txt)
    assert "front_end" not in txt                                                # the example file leaves the default
    if not zero_codeword:
        txt, k = re.subn(r"zero_codeword\s*=\s*true", "zero_codeword   = false", txt)
        assert k == 1
    params = tmp_path / f"ber.ini.bp.{front_end}.{int(zero_codeword)}"
    params.write_text(txt + (f"   front_end = {front_end}\n" if front_end else ""))
    snr = (C.c_double * 32)(); cnt = (C.c_int64 * 160)()
    n = lib.lutldpc_ber_sim_run(str(params).encode(), str(base).encode(), 2, b"", 0, 1, 1, snr, cnt, 32)
    return n, list(snr[:max(n, 0)]), np.array(cnt[:max(n, 0) * 5]).reshape(-1, 5)


def _frame_loop(n, snrs, got, per_frame, nframes=150, K=500):
    """The stop rule of src/LDPC_BER_Sim.cpp:246-311 in frame order over per_frame(i, N0) -> (decided bits XOR sent bits [nframes, N], uncoded
    [nframes])."""
    stop = False
    for i in range(n):
        if stop:
            assert (got[i] == 0).all()
            continue
        bits, unc = per_frame(i, 10 ** (-snrs[i] / 10) / 0.5)
        be = bits[:, :K].sum(1)
        hit = np.flatnonzero(np.cumsum(be > 0) > 20)
        m = int(hit[0]) + 1 if hit.size else nframes
        want = np.array([m, m * K, (be[:m] > 0).sum(), be[:m].sum(), unc[:m].sum()])
        assert (got[i] == want).all(), (i, got[i], want)
        stop = want[3] / want[1] < 1e-7 or want[2] / want[0] < 1e-5


def test_ber_sim_with_the_device_front_end_matches_the_frame_loop(tmp_path):
    """data/params/ber.ini.bp.example with BP.front_end = device (Nframes reduced) through lutldpc_ber_sim_run: the five counters per
    SNR point equal numpy sampler -> oracle decode -> numpy counts with the stop rule in frame order (stream = SNR index, seed =
    rand_seed).  With BP.front_end = host, and with the key absent, the counters are those of the host front end's reference
    (tests/test_30_bp_gpu.py): the default did not move."""
    code = orc.Code(CODES / "rate0.50_dv03_dc06_N1000.alist")
    ref = orc.BP(code, 12, 300, 7, 28)
    ref.set_exit_conditions(30, True, True)

    def device_frames(i, N0):
        q, unc = BC.sample(BC.awgn_table(N0), 2, i, 0, 150, code.nvar)
        return ref.decode_qllr_batch(q)[0], unc

    def host_frames(i, N0):
        llr, unc = orc.awgn_llr(2, i, 0, 150, code.nvar, N0)
        return ref.decode_llr_batch(llr)[0], unc

    n, snrs, got = _run_ber_sim(tmp_path, "device")
    check(min(n, 0))
    assert n == 7 and snrs == [0, .5, 1, 1.5, 2, 2.5, 3] and got[0][2] == 21
    _frame_loop(n, snrs, got, device_frames)
    n_h, snrs_h, got_h = _run_ber_sim(tmp_path, "host")
    check(min(n_h, 0))
    assert n_h == 7
    _frame_loop(n_h, snrs_h, got_h, host_frames)
    n_d, _, got_d = _run_ber_sim(tmp_path, "")
    assert n_d == 7 and (got_d == got_h).all() and (got_h != got).any()
    n_bad, _, _ = _run_ber_sim(tmp_path, "gpu")                                  # any other value is an error
    assert n_bad < 0 and "front_end" in _capi.last_error()


def test_ber_sim_with_the_device_front_end_on_random_codewords(tmp_path):
    """The same file with zero_codeword = false: the driver encodes on the host and hands the bytes to lutldpc_bp_sim_batch.  The
    counters equal numpy sampler (mirrored by the host encoder's codewords) -> oracle decode on the product's column-permuted graph
    -> bit errors against the codeword, with the stop rule in frame order."""
    n, snrs, got = _run_ber_sim(tmp_path, "device", zero_codeword=False)
    check(min(n, 0))
    assert n == 7 and got[0][2] == 21
    pcd = L.Codec(CODES / "rate0.50_dv03_dc06_N1000.alist", with_generator=True, device=-1)
    dv, dc, cn = pcd.graph()
    code = orc.Code(graph=(pcd.nvar, pcd.nchk, dv, dc, cn))
    assert pcd.ninfo == 500
    ref = orc.BP(code, 12, 300, 7, 28)
    ref.set_exit_conditions(30, True, True)

    def frames(i, N0):
        cw = np.stack([pcd.encode(orc.info_bits(2, i, f, 500)) for f in range(150)])
        assert cw.any()
        q, unc = BC.sample(BC.awgn_table(N0), 2, i, 0, 150, code.nvar, cw)
        return ref.decode_qllr_batch(q)[0] ^ cw, unc

    _frame_loop(n, snrs, got, frames)


def test_one_table_many_batch_sizes_then_a_second_table():
    code, N = "n127", 127
    dec = handle(code)
    first, second = BC.awgn_table(*BC.AWGN["awgn_d12"]), BC.awgn_table(*BC.AWGN["awgn_d4"])
    cw = np.random.default_rng(5).integers(0, 256, (513, N), dtype=np.uint8)
    dec.set_cells(first)
    for B in (513, 1, 257, 256, 255, 2, 512):                                    # grows, shrinks, grows: the buffers are reused
        for c in (None, cw[:B]):
            q, unc = dec.sample_qllr(9, 4, 2 ** 32 - 3, B, c)
            wq, wu = BC.sample(first, 9, 4, 2 ** 32 - 3, B, N, c)
            same(q, wq, f"qllr, B = {B}")
            same(unc, wu, f"uncoded, B = {B}")
    dec.set_cells(second)
    q, unc = dec.sample_qllr(9, 4, 2 ** 32 - 3, 257, cw[:257])
    wq, wu = BC.sample(second, 9, 4, 2 ** 32 - 3, 257, N, cw[:257])
    same(q, wq, "qllr, second table")
    same(unc, wu, "uncoded, second table")
    # a refused table leaves the second one in place
    bad = dict(second, qllr=np.full(len(second["qllr"]), BC.QMAX + 1, np.int32))
    with pytest.raises(L.LutLdpcError) as e:
        dec.set_cells(bad)
    assert e.value.code == ERR_ARG
    same(dec.sample_qllr(9, 4, 2 ** 32 - 3, 257, cw[:257])[0], wq, "qllr after a refused table")


def test_refusals_leave_the_outputs_untouched():
    g = BC.graph("n33")
    N = g.nvar
    dec = L.BPDecoder(N, g.nchk, g.dv, g.dc, g.cn_msg_idx, *BC.D, device=0)
    h = dec._h
    q, unc, st, bits = np.full((3, N), 77, np.int32), np.full(3, 77, np.int32), np.full((3, 4), 77, np.int32), np.full((3, N), 77, np.uint8)
    qp, up, sp = (a.ctypes.data_as(C.POINTER(C.c_int32)) for a in (q, unc, st))
    bp = bits.ctypes.data_as(C.POINTER(C.c_uint8))
    S, Q = lib.lutldpc_bp_sample_qllr, lib.lutldpc_bp_sim_batch
    # no table yet: argument errors first, then ERR_STATE
    assert S(h, 1, 2 ** 31, 0, 3, None, qp, up) == ERR_ARG and S(h, 1, 0, 0, 3, None, None, up) == ERR_ARG and S(h, 1, 0, 0, 0, None, qp, up) == ERR_ARG
    assert S(h, 1, 0, 0, 3, None, qp, up) == ERR_STATE and "table" in _capi.last_error()
    assert Q(h, 1, 0, 0, 3, None, N + 1, sp, qp, bp) == ERR_ARG and Q(h, 1, 0, 0, 3, None, 5, None, qp, bp) == ERR_ARG
    assert Q(h, 1, 0, 0, 3, None, 5, sp, qp, bp) == ERR_STATE and "table" in _capi.last_error()
    # refused tables on a device handle: still no table afterwards
    good = BC.named([1 << 62, 1 << 63])
    for t in (dict(good, thr=np.array([1 << 63, 1 << 62], np.uint64)), dict(good, qllr=np.array([0, -BC.QMAX - 1, 0], np.int32))):
        assert lib.lutldpc_bp_set_cells(h, C.byref(_capi.BPCells.from_table(t))) == ERR_ARG
    c = _capi.BPCells.from_table(good)
    c.n_cells = 0
    assert lib.lutldpc_bp_set_cells(h, C.byref(c)) == ERR_ARG and lib.lutldpc_bp_set_cells(h, None) == ERR_ARG
    assert Q(h, 1, 0, 0, 3, None, 5, sp, qp, bp) == ERR_STATE
    # with a table: the argument errors remain, the good call goes through
    dec.set_cells(good)
    assert S(h, 1, 2 ** 31, 0, 3, None, qp, up) == ERR_ARG and S(h, 1, 0, 0, -1, None, qp, up) == ERR_ARG and S(h, 1, 0, 0, 3, None, None, up) == ERR_ARG
    assert Q(h, 1, 2 ** 31, 0, 3, None, 5, sp, qp, bp) == ERR_ARG and Q(h, 1, 0, 0, 3, None, -1, sp, qp, bp) == ERR_ARG
    assert Q(h, 1, 0, 0, 0, None, 5, sp, qp, bp) == ERR_ARG and Q(None, 1, 0, 0, 3, None, 5, sp, qp, bp) == ERR_ARG
    assert (q == 77).all() and (unc == 77).all() and (st == 77).all() and (bits == 77).all()
    assert S(h, 1, 2 ** 31 - 1, 0, 3, None, qp, None) == 0 and (unc == 77).all()              # uncoded_out is optional
    same(q, BC.sample(good, 1, 2 ** 31 - 1, 0, 3, N)[0], "qllr at the largest stream")
    dec.close()
