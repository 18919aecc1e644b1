"""Per-node channel classes of the sampler without a GPU: the argument-error order of both setters on host-only handles, the class
tables of the codec layer (finite offsets and the two limits, punctured and known) through lutldpc_codec_node_channel_cells, the
errors of the two ber_sim keys, each naming its key, and the [BP] refusal.  And, with the reference and the oracle alone, the
conditions the cases of tests/node_channel_cases.py are built for, so that no test of tests/test_33_node_channels_gpu.py passes
empty: every class of every case receives samples, both cells of an erasure class are hit under a sent 0 and a sent 1, every decode
batch holds a frame that converges and one that does not."""
import ctypes as C

import numpy as np
import pytest

import frontend_cases as fc
import node_channel_cases as nc
import lut_ldpc_amd as L
from lut_ldpc_amd._capi import ERR_ARG, ERR_STATE, ChannelCells, LutLdpcError, NodeChannels, last_error, lib
from helpers import CODES, oracle_codec, product_decoder

INF = float("inf")


# ---------------------------------------------------------------------------------------------------------------- decoder setter
@pytest.fixture(scope="module")
def host_only():
    cd = oracle_codec("n500_q4_i8")
    dec = product_decoder(cd, device=-1)
    table = {k: np.ascontiguousarray(v) for k, v in cd.channel_cells(2.0, cd.rate).items()}
    yield dec, table, cd
    dec.close()


def _bad(table, **kw):
    t = dict(table)
    t.update(kw)
    return t


def test_decoder_setter_checks_its_arguments_before_the_device(host_only):
    dec, table, cd = host_only
    N = dec.nvar
    ids = (np.arange(N) % 2).astype(np.uint8)
    call = lambda rec: lib.lutldpc_decoder_set_node_channels(dec._h, C.byref(rec) if rec is not None else None)
    assert lib.lutldpc_decoder_set_node_channels(None, C.byref(NodeChannels.from_tables(ids, [table, table]))) == ERR_ARG
    for n in (-1, 17):
        rec = NodeChannels.from_tables(ids, [table, table])
        rec.n_classes = n
        assert call(rec) == ERR_ARG and "n_classes" in last_error(), n
    for member in ("tables", "node_class"):
        rec = NodeChannels.from_tables(ids, [table, table])
        setattr(rec, member, None)
        assert call(rec) == ERR_ARG and "NULL member" in last_error(), member
    # every table goes through the check of the `cells` of sim_batch
    two = np.array([5, 4], np.uint64)
    for bad, text in ((_bad(table, thr=np.concatenate([two, table["thr"][2:]])), "ascend"), (_bad(table, cha=np.full_like(table["cha"], cd.nq_cha)), "alphabet"),
                      (_bad(table, msg_m=np.full_like(table["msg_m"], cd.nq_msg[0])), "alphabet")):
        assert call(NodeChannels.from_tables(ids, [table, bad])) == ERR_ARG and text in last_error(), text
    cells = ChannelCells.from_table(table)
    cells.n_cells = 73
    assert call(NodeChannels.from_tables(ids, [table, cells])) == ERR_ARG and "n_cells" in last_error()
    cells = ChannelCells.from_table(table)
    cells.slicer_neg = None
    assert call(NodeChannels.from_tables(ids, [cells, table])) == ERR_ARG and "NULL member" in last_error()
    over = ids.copy()
    over[N - 1] = 2
    assert call(NodeChannels.from_tables(over, [table, table])) == ERR_ARG and f"node_class[{N - 1}]" in last_error()
    # valid arguments, 16 classes and a class without a node among them: the handle has no device
    assert call(NodeChannels.from_tables(ids, [table] * 16)) == ERR_STATE and "host-only handle" in last_error()
    assert call(NodeChannels.from_tables(ids, [table, table])) == ERR_STATE
    assert call(None) == ERR_STATE                                        # clearing is a call like any other
    with pytest.raises(LutLdpcError, match="host-only handle"):
        dec.set_node_channels(ids, [table, table])
    with pytest.raises(ValueError):
        dec.set_node_channels(ids[:-1], [table, table])
    assert "node_channels" not in dec.describe()
    # NULL cells without node channels on a host-only handle stays a state error (tests/test_entry_guards_cpu.py holds that too)
    out = np.zeros((3, N), np.uint8)
    p = out.ctypes.data_as(C.POINTER(C.c_uint8))
    assert lib.lutldpc_decoder_sample_labels(dec._h, None, 7, 1, 0, 3, None, p, p) == ERR_STATE


# ---------------------------------------------------------------------------------------------------------------- codec layer
def _codec(nq_cha=16, nq_msg=16, mode=0, iters=2):
    cd = L.Codec(CODES / "rate0.50_dv02-17_dc08-09_lut_q4_N500.alist", known_rank=250, device=-1)
    cd.design_luts(sigma2=0.88 ** 2, max_iters=iters, nq_cha=nq_cha, nq_msg=nq_msg)
    cd.set_initial_message_mode(mode)
    return cd


def test_codec_setter_checks_its_arguments_and_works_on_a_host_only_codec():
    cd = _codec()
    N = cd.nvar
    ids = (np.arange(N) % 4).astype(np.uint8)
    off = np.array([0.0, -INF, INF, -3.0])
    u8, dp = C.POINTER(C.c_uint8), C.POINTER(C.c_double)
    call = lambda h, i, n, o: lib.lutldpc_codec_set_node_channels(h, i.ctypes.data_as(u8) if i is not None else None, n, o.ctypes.data_as(dp) if o is not None else None)
    assert call(None, ids, 4, off) == ERR_ARG
    for n in (-1, 17):
        assert call(cd._h, ids, n, np.zeros(17)) == ERR_ARG and "classes" in last_error()
    assert call(cd._h, None, 4, off) == ERR_ARG and call(cd._h, ids, 4, None) == ERR_ARG
    assert call(cd._h, ids, 4, np.array([0.0, float("nan"), 1.0, 2.0])) == ERR_ARG and "not a number" in last_error()
    assert call(cd._h, ids, 3, off) == ERR_ARG and "class 3" in last_error()
    # nothing was set by the refused calls
    with pytest.raises(LutLdpcError, match="classes set"):
        cd.node_channel_cells(2.0, 0)
    cd.set_node_channels(ids, off)
    assert len(cd.node_channel_cells(2.0, 3)["cha"]) > 2
    with pytest.raises(LutLdpcError, match="classes set"):
        cd.node_channel_cells(2.0, 4)
    # a refused call leaves the setting in place; the entries that sample reach the decoder's setter: no device
    assert call(cd._h, ids, 2, off) == ERR_ARG
    assert len(cd.node_channel_cells(2.0, 3)["cha"]) > 2
    with pytest.raises(LutLdpcError, match="host-only handle"):
        cd.sim_batch(2.0, 7, 1, 0, 3)
    cd.set_node_channels(None)
    with pytest.raises(LutLdpcError, match="classes set"):
        cd.node_channel_cells(2.0, 0)
    with pytest.raises(ValueError):
        cd.set_node_channels(ids[:-1], off)
    cd.close()


@pytest.mark.parametrize("nq_cha,nq_msg,mode", [(16, 16, 0), (16, 16, 1), (16, 8, 1), (6, 6, 0), (14, 10, 1), (2, 4, 0)],
                         ids=["cont", "qcha", "qcha-m8", "odd-half-cont", "odd-half-qcha", "hard-channel"])
def test_class_tables_of_the_codec_finite_offsets_and_both_limits(nq_cha, nq_msg, mode):
    """Class 0 (offset 0) is the code's own table, a finite offset the code's table at snr + offset, -inf and +inf the two tables the
    header states -- in CONT and QCHA mode and on alphabets whose half is odd.  The designed quantisers are symmetric, so one boundary
    lies AT zero: the two erasure cells differ in < 0 against <= 0."""
    cd = _codec(nq_cha, nq_msg, mode)
    N = cd.nvar
    cd.set_node_channels((np.arange(N) % 4).astype(np.uint8), [0.0, -INF, INF, -3.0])
    qc, qm, mp = cd.qb_cha, cd.qb_msg, cd.cha2msg_map
    assert len(qc) == nq_cha - 1
    assert (qc == 0).sum() == 1 and (qc < 0).sum() == nq_cha // 2 - 1
    for snr in (1.5, 4.0):
        assert nc.same_table(cd.node_channel_cells(snr, 0), cd.channel_cells(snr))
        assert nc.same_table(cd.node_channel_cells(snr, 3), cd.channel_cells(snr - 3.0))
        assert not nc.same_table(cd.node_channel_cells(snr, 3), cd.channel_cells(snr))
        want_e = nc.erasure_table(qc, qm if mode == 0 else None, mp if mode == 1 else None)
        want_k = nc.known_table(qc, qm if mode == 0 else None, mp if mode == 1 else None)
        got_e, got_k = cd.node_channel_cells(snr, 1), cd.node_channel_cells(snr, 2)
        assert nc.same_table(got_e, want_e), (got_e, want_e)
        assert nc.same_table(got_k, want_k), (got_k, want_k)
        assert len(got_e["cha"]) == 2 and got_e["thr"].tolist() == [1 << 63] and got_e["neg"].tolist() == [1, 0]
        assert len(got_k["cha"]) == 1 and got_k["cha"][0] == nq_cha - 1 and got_k["cha_m"][0] == 0 and got_k["neg"][0] == 0
    # the erasure is the limit of the finite tables: at a very low SNR the cells around zero hold all the mass and carry those labels
    cd.set_node_channels((np.arange(N) % 2).astype(np.uint8), [-400.0, 400.0])
    low, high = cd.node_channel_cells(2.0, 0), cd.node_channel_cells(2.0, 1)
    mass = np.diff(np.concatenate([[0], low["thr"].astype(object), [1 << 64]]))
    heavy = [j for j, m in enumerate(mass) if m > (1 << 62)]
    assert len(heavy) == 2 and [int(low["cha"][j]) for j in heavy] == want_e["cha"].tolist() and [int(low["neg"][j]) for j in heavy] == [1, 0], heavy
    assert [int(low["msg"][j]) for j in heavy] == want_e["msg"].tolist()
    top = len(high["cha"]) - 1
    assert all(int(t) == 0 for t in high["thr"]) and high["cha"][top] == want_k["cha"][0] and high["msg"][top] == want_k["msg"][0] and high["neg"][top] == 0
    cd.close()


# ---------------------------------------------------------------------------------------------------------------- ber_sim keys
def _create(params, base):
    h = C.c_void_p()
    rc = lib.lutldpc_bersim_create(str(params).encode(), str(base).encode(), 0, b"", -1, C.byref(h))
    msg = last_error()
    if rc == 0:
        lib.lutldpc_bersim_destroy(h)
    return rc, msg


def test_ber_sim_keys_are_checked_and_every_error_names_its_key(tmp_path):
    ok, base = nc.write_ber_case(tmp_path)
    assert _create(ok, base)[0] == 0
    assert _create(nc.write_ber_case(tmp_path, channel=False, name="plain.ini")[0], base)[0] == 0
    # one key without the other
    for keep, missing in (("node_classes_filename", "class_snr_offset_dB"), ("class_snr_offset_dB", "node_classes_filename")):
        p = tmp_path / f"only_{keep}.ini"
        p.write_text("\n".join(line for line in ok.read_text().splitlines() if missing not in line) + "\n")
        rc, msg = _create(p, base)
        assert rc != 0 and f"Channel.{missing}" in msg and "missing" in msg, msg
    cases = [
        (dict(offsets=["0", "-inf", "inf"]), "Channel.class_snr_offset_dB"),                 # an id outside the offsets
        (dict(offsets=["0", "nan", "inf", "-3"]), "Channel.class_snr_offset_dB"),
        (dict(offsets=["0", "minus", "inf", "-3"]), "Channel.class_snr_offset_dB"),
        (dict(offsets=["0"] * 17), "Channel.class_snr_offset_dB"),
        (dict(classes=nc.ber_classes()[:-1]), "Channel.node_classes_filename"),             # a wrong count
        (dict(classes=np.concatenate([nc.ber_classes(), [0]])), "Channel.node_classes_filename"),
    ]
    for i, (kw, key) in enumerate(cases):
        p, b = nc.write_ber_case(tmp_path, name=f"bad{i}.ini", **kw)
        rc, msg = _create(p, b)
        assert rc != 0 and key in msg, (kw, msg)
    nc.write_ber_case(tmp_path)                                                             # (the class file as it was)
    (base / "codes" / "classes.txt").write_text("0 1 x 2\n")
    rc, msg = _create(ok, base)
    assert rc != 0 and "Channel.node_classes_filename" in msg and "'x'" in msg
    (base / "codes" / "classes.txt").unlink()
    rc, msg = _create(ok, base)
    assert rc != 0 and "Channel.node_classes_filename" in msg and "cannot open" in msg


def test_bp_simulations_refuse_the_keys(tmp_path):
    p, base = nc.write_ber_case(tmp_path, section="BP")
    rc, msg = _create(p, base)
    assert rc != 0 and "[BP]" in msg and "Channel.node_classes_filename" in msg, msg
    p, base = nc.write_ber_case(tmp_path, channel=False, section="BP", name="bp_plain.ini")
    assert _create(p, base)[0] == 0


# ---------------------------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("case", nc.CASES, ids=nc.case_id)
def test_every_class_of_every_case_receives_samples_and_the_tables_differ(case):
    c = nc.sampler_case(case)
    cls, tables, N, B = c["node_class"], c["tables"], c["N"], c["B"]
    count = np.bincount(cls, minlength=len(tables))
    layout = case[1]
    assert ((count > 0) | (np.arange(len(tables)) == 1)).all() if layout == "empty" else (count > 0).all(), count
    assert B >= 1 and len(cls) == N
    cha, msg, unc, _ = nc.reference(case, "none")
    for sent in ("bytes", "device"):
        cha1, msg1, unc1, cw = nc.reference(case, sent)
        assert (unc1 == unc).all()                                          # the slicer column does not look at the sent bit
        assert cw.shape == (B, N) and (cw & 1).any() and not (cw & 1).all()
        assert (cha1 != cha).any() or (msg1 != msg).any()
    if len(tables) > 1:
        # a sampler that used class 0's table on every node would be caught: the one-table labels differ from the reference
        one_cha, one_msg, _ = fc.sample(tables[0], c["seed"], c["stream"], c["f0"], B, N, None, u=c["u"])
        assert (one_cha != cha).any() or (one_msg != msg).any()
        # and so would one that took the class of the pair's first node for both nodes
        pair = cls.copy()
        pair[1::2] = cls[0:N - 1:2][:len(pair[1::2])]
        if (pair != cls).any():
            p_cha, p_msg, _ = nc.sample(tables, pair, c["seed"], c["stream"], c["f0"], B, N, None, u=c["u"])
            assert (p_cha != cha).any() or (p_msg != msg).any() or B * N < 64


def test_the_cases_cover_what_they_are_for():
    sizes = {len(t["cha"]) for case in nc.CASES if case[1] == "mod16" for t in nc.sampler_case(case)["tables"]}
    assert {1, 2, 35, 72} <= sizes
    assert all(len(nc.sampler_case(case)["tables"]) == 16 for case in nc.CASES if case[1] == "mod16")
    assert {case[1] for case in nc.CASES} == set(nc.LAYOUTS)
    assert {nc.HANDLES[case[0]][2] for case in nc.CASES} == {256, 512}                  # byte and nibble rows
    assert {case[0].split("_")[0] for case in nc.CASES} == {"n127", "n33"}
    assert {case[2] for case in nc.CASES} == {"1", "T-1", "T", "T+1", "2T+3"}
    assert any(case[3] == fc.F_CARRY for case in nc.CASES) and any(case[3] == fc.F_WRAP and nc.sampler_case(case)["B"] >= 12 for case in nc.CASES)
    for N in (127, 33):
        blocks = nc.node_classes("blocks", N)
        assert blocks[4] != blocks[5] and (blocks == 3).sum() == 1 and blocks[N - 1] == 3 and len(set(blocks[:nc.WAVE_NODES])) == 2
        assert set(nc.node_classes("empty", N)) == {0, 2}
        assert (nc.node_classes("evenodd", N)[0::2] == 0).all() and (nc.node_classes("evenodd", N)[1::2] == 1).all()


@pytest.mark.parametrize("handle,bk,snr_a,snr_b", nc.STATS_CASES, ids=[c[0] for c in nc.STATS_CASES])
@pytest.mark.parametrize("sent", ["bytes", "device"])
def test_decode_batches_hold_both_outcomes_and_the_erasure_class_hits_both_cells(handle, bk, snr_a, snr_b, sent):
    ref = nc.stats_reference(handle, bk, snr_a, snr_b, sent)
    assert (ref["iters"] >= 0).any() and (ref["iters"] < 0).any(), ref["iters"]
    cls, cw, cha = ref["node_class"], ref["cw"] & 1, ref["cha"]
    assert (np.bincount(cls, minlength=4) > 0).all()
    era, tab = cha[:, cls == 1], ref["tables"][1]
    bit = cw[:, cls == 1].astype(bool)
    assert bit.any() and (~bit).any()
    # sent 0: the labels of cell 0 and of cell 1; sent 1: their mirrors -- all four occur
    assert set(era[~bit].tolist()) == set(tab["cha"].tolist()) and set(era[bit].tolist()) == set(tab["cha_m"].tolist())
    assert tab["cha"][0] != tab["cha"][1]
    known = cha[:, cls == 2]
    assert set(known[~cw[:, cls == 2].astype(bool)].tolist()) == {int(ref["tables"][2]["cha"][0])}
    assert (ref["unc"] > 0).any()


def test_the_punctured_example_loads_with_its_class_file(tmp_path):
    import shutil
    from helpers import ROOT
    (tmp_path / "codes").mkdir()
    for f in CODES.glob("rate0.50_dv02-17_dc08-09_lut_q4_N500.*"):
        shutil.copy(f, tmp_path / "codes")
    rc, msg = _create(ROOT / "data" / "params" / "ber.ini.punctured.example", tmp_path)
    assert rc == 0, msg
    cls = np.array((CODES / "rate0.50_dv02-17_dc08-09_lut_q4_N500.punctured.classes").read_text().split(), int)
    assert len(cls) == 500 and np.bincount(cls).tolist() == [400, 50, 50]
