"""The references of tests/frontend_cases.py, without a GPU: the numpy Philox4x32-10 against the published known answers; the oracle's
information bits and cell sampler (oracle/or_sim.c) against the numpy references on real cell tables, over the batch geometry of the
GPU cases (carry into the high frame word, the 2^64 wrap); every crafted cell table against the condition it is for, under the
reference alone; the host encoder against the reference encoder."""
import numpy as np
import pytest

import frontend_cases as fc
from oracle import oracle as orc


def test_numpy_philox_reproduces_the_published_known_answers():
    for ctr, key, want in fc.KNOWN_ANSWERS:
        got = fc.philox4x32_10(*ctr, *key)
        assert tuple(int(x) for x in got) == want, [hex(int(x)) for x in got]
    # vectorised: the three at once, as arrays
    c = [np.array([ka[0][i] for ka in fc.KNOWN_ANSWERS], np.uint64) for i in range(4)]
    k = [np.array([ka[1][i] for ka in fc.KNOWN_ANSWERS], np.uint64) for i in range(2)]
    got = np.stack(fc.philox4x32_10(*c, *k), axis=1)
    assert (got == np.array([ka[2] for ka in fc.KNOWN_ANSWERS], np.uint64)).all()


def test_uniform_layout_of_the_reference():
    """Node 2p takes words (1, 0) and node 2p + 1 words (3, 2) of block p; an odd N drops the second half of the last block; the
    frame index is taken mod 2^64."""
    seed, stream, f0, B, N = fc.SEED_BIG, 7, fc.F_WRAP, 12, 33
    u = fc.uniforms(seed, stream, f0, B, N)
    assert u.shape == (B, N) and u.dtype == np.uint64
    for i, v in [(0, 0), (4, 32), (5, 0), (11, 31), (6, 17)]:
        f = (f0 + i) % 2 ** 64
        c = fc.philox4x32_10(f & 0xFFFFFFFF, f >> 32, v // 2, stream, seed & 0xFFFFFFFF, seed >> 32)
        want = (int(c[3]) << 32 | int(c[2])) if v % 2 else (int(c[1]) << 32 | int(c[0]))
        assert int(u[i, v]) == want
    assert fc.frames(f0, B).tolist() == [2 ** 64 - 5 + i for i in range(5)] + list(range(7))
    assert (fc.uniforms(seed, stream, 0, 7, N) == u[5:]).all()                         # frames are addressable across the wrap
    assert (fc.uniforms(seed, stream, f0, B, 34)[:, :33] == u).all()


@pytest.mark.parametrize("seed,stream,f0", [(3, 0, 0), (fc.SEED_BIG, 7, fc.F_CARRY), (3, fc.STREAM_MAX, fc.F_HIGH), (fc.SEED_BIG, 0, fc.F_WRAP)])
def test_oracle_info_bits_equal_the_reference(seed, stream, f0):
    B = 12
    for K in (1, 31, 32, 33, 127, 128, 129, 500, 8192):
        want = fc.info_bits(seed, stream, f0, B, K)
        assert want.shape == (B, K)
        for i in range(B):
            assert (orc.info_bits(seed, stream, (f0 + i) % 2 ** 64, K) == want[i]).all(), (K, i)
    assert 0.4 < fc.info_bits(seed, stream, f0, B, 8192).mean() < 0.6


def test_why_a_stream_with_bit_31_is_refused():
    """With stream = s | 2^31 the channel uniforms of pair p would be the Philox block that makes information bits 128p .. 128p + 127
    of stream s, and both streams would send the same data: stated here with the references (the entries refuse such a stream:
    tests/test_entry_guards_cpu.py, tests/test_21_frontend_limits_gpu.py)."""
    seed, s, f0, B, N = fc.SEED_BIG, 7, fc.F_CARRY, 9, 10
    u = fc.uniforms(seed, s | 2 ** 31, f0, B, N)
    bits = fc.info_bits(seed, s, f0, B, 128 * (N // 2))
    as_bits = ((u[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).reshape(B, -1).astype(np.uint8)
    assert (as_bits == bits).all()
    assert (fc.info_bits(seed, s | 2 ** 31, f0, B, 300) == fc.info_bits(seed, s, f0, B, 300)).all()
    assert (fc.uniforms(seed, fc.STREAM_MAX, f0, B, N) != fc.uniforms(seed, fc.STREAM_MAX | 2 ** 31, f0, B, N)).all()


# (handle of frontend_cases.HANDLES, SNR in dB) of the real tables; every (batch size, frame0, seed, stream) of the sampler cases on them
REAL = [("q4", 2.0), ("q5", 2.0), ("n127", 0.0), ("n33", 3.0), ("q4", fc.DENSE_SNR), ("q6", fc.DENSE_SNR)]
GEOMETRY = [("1", 0, 3, 0), ("T-1", fc.F_CARRY, fc.SEED_BIG, 7), ("T", fc.F_HIGH, 3, fc.STREAM_MAX), ("T+1", fc.F_WRAP, fc.SEED_BIG, 0),
            ("2T+3", fc.F_CARRY, 3, 7), ("T-1", fc.F_WRAP, 3, fc.STREAM_MAX)]


def test_geometry_holds_every_value_of_the_issue():
    assert {c[2] for c in fc.SAMPLER_CASES} == {"1", "T-1", "T", "T+1", "2T+3"}
    assert {c[3] for c in fc.SAMPLER_CASES} >= {0, fc.F_CARRY, fc.F_HIGH, fc.F_WRAP}
    assert {c[4] for c in fc.SAMPLER_CASES} == {3, fc.SEED_BIG} and {c[5] for c in fc.SAMPLER_CASES} == {0, 7, fc.STREAM_MAX}
    assert {c[1] for c in fc.SAMPLER_CASES} == set(fc.TABLES)
    odd, nibble, byte = ("n127", "n127_pack1", "n33"), ("q4", "n127", "n33"), ("q4_pack1", "q5", "q6", "n127_pack1")
    for t in fc.TABLES:
        mine = [c for c in fc.SAMPLER_CASES if c[1] == t]
        assert any(c[2] in ("T-1", "T+1", "2T+3") for c in mine), t
        assert any(c[0] in byte for c in mine), t
        if t != "dense_q6":                                # (64 labels: byte rows only, and only on the 64-label handle)
            assert any(c[0] in odd for c in mine) and any(c[0] in nibble for c in mine), t
    for c in fc.SAMPLER_CASES:
        if c[3] == fc.F_WRAP:
            assert fc.batch_size(c[2], fc.HANDLES[c[0]][2]) >= 12, c
    assert fc.codec("n127").code.nvar == 127 and fc.codec("n33").code.nvar == 33
    assert sorted(set(fc.codec("n127").code.dc.tolist())) == [3, 6] and set(fc.codec("n33").code.dv.tolist()) == {2}


@pytest.mark.parametrize("handle,snr", REAL)
def test_oracle_sampler_equals_the_reference_on_real_tables(handle, snr):
    code, _, T = fc.HANDLES[handle]
    cd = fc.codec(code)
    cd.set_initial_message_mode(0)
    N = cd.code.nvar
    cells = cd.channel_cells(snr, cd.rate)
    rng = np.random.default_rng(N)
    for bk, f0, seed, stream in GEOMETRY:
        B = fc.batch_size(bk, T)
        u = fc.uniforms(seed, stream, f0, B, N)
        for cw in (None, rng.integers(0, 2, (B, N), dtype=np.uint8), np.ones((B, N), np.uint8)):
            want = fc.sample(cells, seed, stream, f0, B, N, cw, u=u)
            got = cd.sample_labels(snr, cd.rate, seed, stream, f0, B, codewords=cw)
            for w, g, what in zip(want, got, ("cha", "msg", "uncoded")):
                assert (w == g).all(), (what, bk, f0, seed, stream, None if cw is None else int(cw.sum()))
    if snr < fc.DENSE_SNR:
        assert want[2].any()


def test_real_dense_tables_are_the_products_and_as_dense_as_stated():
    from helpers import product_codec
    for name, (cfg, dense) in fc.REAL_DENSE.items():
        cells = fc.real_dense(name)
        pcd = product_codec(cfg)
        pcd.set_initial_message_mode(0)
        got = pcd.channel_cells(fc.DENSE_SNR)
        pcd.close()
        for k in cells:
            assert (cells[k] == got[k]).all(), (name, k)
        assert fc.thresholds_per_slice(cells).max() == dense, (name, fc.thresholds_per_slice(cells).max())


@pytest.mark.parametrize("case", fc.SAMPLER_CASES, ids=fc.case_id)
def test_every_table_meets_its_condition_under_the_reference(case):
    handle, table, bk, f0, seed, stream = case
    cells, u, N, B, T, cw01, cw_bytes = fc.sampler_case(case)
    n = len(cells["cha"])
    cd = fc.codec(fc.HANDLES[handle][0])
    assert (cells["cha"] < cd.nq_cha).all() and (cells["cha_m"] < cd.nq_cha).all() and (cells["msg"] < cd.nq_msg[0]).all() and (cells["msg_m"] < cd.nq_msg[0]).all()
    thr = cells["thr"][:n - 1]
    assert all(a <= b for a, b in zip(thr[:-1], thr[1:]))
    cell = fc.cells_of(cells, u)
    hit = np.bincount(cell.ravel(), minlength=n)
    assert len(hit) == n
    if table not in fc.REAL_DENSE:
        # the labels name the cell, for a sent 0 and for a sent 1, and the slicer column is not monotone
        assert len({(a, m) for a, m in zip(cells["cha"], cells["msg"])}) == n and len({(a, m) for a, m in zip(cells["cha_m"], cells["msg_m"])}) == n
        if n > 2:
            assert (cells["cha"] != cells["cha_m"]).any() and {1, -1} <= set(np.diff(cells["neg"].astype(int)).tolist())
    assert (cw_bytes & 1).tolist() != cw01.tolist() and (cw_bytes > 1).any()
    if table == "pins":
        assert n == 72
        picks = fc.pin_samples(B, N, T, f0)
        assert len(picks) == len(set(picks)) == 35
        fr, nodes = {i for i, _ in picks}, {v for _, v in picks}
        F = T // 64
        assert {0, B - 1} <= fr and {0, N - 1} <= nodes
        if B > F:
            assert {F - 1, F} <= fr
        if B > T:
            assert {T - 1, T} <= fr
        if f0 in (fc.F_CARRY, fc.F_WRAP):
            w = 2 ** 32 - f0 % 2 ** 32
            assert {w - 1, w} <= fr and (f0 + w) % 2 ** 32 == 0
        pinned = set()
        for i, v in picks:
            c = int(cell[i, v])
            assert int(thr[c - 1]) == int(u[i, v]) and int(thr[c]) == int(u[i, v]) + 1          # the cell [u, u + 1)
            assert hit[c] == (u == u[i, v]).sum() >= 1
            pinned.add(c)
        assert len(pinned) == 35
    elif table == "one_bucket":
        assert n == 72 and len(set((thr >> np.uint64(64 - fc.BUCKET_BITS)).tolist())) == 1
        assert fc.thresholds_per_slice(cells).max() == 71
        assert (hit > 0).all()
        assert np.isin(u, thr).sum() >= 71 and np.isin(thr, u).all()
    elif table == "boundaries":
        t, empty = fc.table_boundaries()
        assert t == [int(x) for x in thr]
        assert 0 in empty and n - 1 in empty and len(empty) == 2 + 2 * len(fc.BOUNDARY_KS) + 2
        assert sorted(np.flatnonzero(hit == 0).tolist()) == empty, (np.flatnonzero(hit == 0), empty)
        for k in (1, 1023):
            assert k << 54 in t and (k << 54) - 1 in t and (k << 54) + 1 in t
        assert t[0] == 0 and t[-1] == 2 ** 64 - 1 and max(t.count(x) for x in t) == 3
    elif table == "trivial1":
        assert n == 1 and len(cells["thr"]) == 1 and (cell == 0).all()
    elif table == "trivial2":
        assert n == 2 and int(thr[0]) == 1 << 63 and hit.min() > 0
    else:
        assert fc.thresholds_per_slice(cells).max() == fc.REAL_DENSE[table][1]


def test_stats_cases_show_frames_with_and_without_data_bit_errors():
    """The counters case (frontend_cases.STATS_CASES): with the oracle decoding the reference's labels, the frames of the batch
    split into both kinds at every K_info > 0, the iteration codes vary and the slicer errs."""
    for handle, Ks in fc.STATS_CASES[:1] + fc.STATS_CASES[2:]:
        ref = fc.stats_reference(handle, "T+1", oracle_frames=None)
        assert Ks[0] == 0 and Ks[-1] == ref["N"] and Ks[-2] == ref["N"] - 1
        for K in Ks[1:]:
            err = (ref["bits"][:, :K] ^ (ref["cw"][:, :K] & 1)).sum(1)
            assert (err > 0).any() and (err == 0).any(), (handle, K, int((err > 0).sum()))
        assert len(set(ref["iters"].tolist())) > 3 and (ref["iters"] < 0).any() and (ref["unc"] > 0).any()
        assert (ref["cw"] > 1).any() and (ref["cw"] & 1).any()


def test_generator_references_mask_the_bits_beyond_k():
    for K, R in ((1, 999), (33, 967), (129, 871), (64, 63)):
        rows = fc.generator_rows(K, R)
        assert rows.shape == (R, (K + 63) // 64)
        if K % 64:
            assert (rows[:, -1] >> np.uint64(K % 64)).all()                       # every row carries bits at positions >= K
        A = fc.generator_bits(rows, K)
        assert A.shape == (R, K) and 0.3 < A.mean() < 0.7
        u = fc.info_bits(5, 1, 0, 9, K)
        cw = fc.encode(A, u)
        assert cw.dtype == np.int64 and cw.shape == (9, K + R) and (cw[:, :K] == u).all()
        assert (cw[:, K:] == (A.astype(np.int64) @ u.T.astype(np.int64)).T % 2).all()
    assert fc.encode(fc.generator_bits(fc.generator_rows(1000, 0), 1000), fc.info_bits(5, 1, 0, 3, 1000)).shape == (3, 1000)
    assert fc.GENERATOR_REFUSED[1] == 8193 and ("n10000", 8192, 1808) in fc.GENERATOR_CASES


def test_host_encoder_equals_the_reference_encoder():
    """Codec(device=-1, with_generator=True).encode against the reference encode() with the codec's own generator, read off the
    encoder column by column (the codeword of unit vector k is column k), on the reference's information bits; every codeword
    satisfies the graph's checks.  The host's random_info_bits is reached only through sample_labels(zero_codeword=False), which a
    host-only handle refuses (it ends in the device sampler): that path is held on the GPU, in tests/test_40_device_codewords_gpu.py
    and tests/test_21_frontend_limits_gpu.py."""
    import lut_ldpc_amd as L
    from helpers import CODES
    pcd = L.Codec(CODES / "rate0.50_dv02-17_dc08-09_lut_q4_N500.alist", with_generator=True, device=-1)
    K, N = pcd.ninfo, pcd.nvar
    with pytest.raises(L.LutLdpcError):
        pcd.sample_labels(2.0, 1, 0, 0, 2, zero_codeword=False)
    unit = np.stack([pcd.encode(np.eye(K, dtype=np.uint8)[k]) for k in range(K)])
    assert (unit[:, :K] == np.eye(K, dtype=np.uint8)).all()
    A = unit[:, K:].T                                                             # R x K
    u = fc.info_bits(fc.SEED_BIG, 7, fc.F_CARRY, 40, K)
    want = fc.encode(A, u)
    dv, dc, cn = pcd.graph()
    H = np.zeros((pcd.nchk, N), np.int64)
    H[np.repeat(np.arange(pcd.nchk), dc), np.repeat(np.arange(N), dv)[cn]] = 1
    for i in range(len(u)):
        assert (pcd.encode(u[i]) == want[i]).all(), i
    assert not ((H @ want.T) % 2).any()
    pcd.close()
