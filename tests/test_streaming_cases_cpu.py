"""The streaming pass kernels' degree sweep (tests/streaming_cases.py) without a GPU.  What tests/test_08_streaming_degrees_gpu.py
reaches is computed here, not claimed: from the case list and describe() on host-only handles, the degrees under the per-class
kernels and under every bucket of the fused kernel, in nibble and in byte rows, plain and chained, are the whole range the kernels
are compiled for -- and every code of the tables is needed for that.  And with the oracle alone: every batch holds frames that
converge at different iterations and frames that do not converge, so equal outputs mean equal decoders."""
import pytest

import streaming_cases as sc

SWEEP_CODES = [n for n in sc.SWEEP if n != sc.WIDE_LABELS]


@pytest.fixture(scope="module")
def described():
    """describe() of every case of sections A to C on a host-only handle: {case id: (code, knobs, description)}."""
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        for cid, name, kn, _ in sc.CASES:
            dec, desc = sc.describe(name, kn, mp)
            dec.close()
            out[cid] = (name, kn, desc)
    return out


def _reached(described, codes, pack):
    """The (kind, degree, bucket) bodies the cases of these codes reach at this row format."""
    out = set()
    for name, _, desc in described.values():
        if name in codes and desc["pack"] == pack:
            out |= {b[:3] for b in sc.bodies(desc)}
    return out


def _sweep_gaps(described, codes, pack):
    """What the sweep codes leave out: per-class bodies of every degree, and every degree a bucket holds in its fused kernel."""
    got = _reached(described, codes, pack)
    want = {("VAR", d, None) for d in sc.VN_DEGREES} | {("DEC", d, None) for d in sc.VN_DEGREES} | {("CHK", d, None) for d in sc.CN_DEGREES}
    for b in sc.BUCKET_ORDER:
        want |= {("VAR", d, b) for d in range(1, sc.FUSED_VN_DEG[b] + 1)} | {("CHK", d, b) for d in range(2, sc.FUSED_CN_DEG[b] + 1)}
    return want - got


def _chain_gaps(described, codes, pack):
    """What the zigzag codes leave out: the chained check body of every degree 3..32 in the bucket the code runs in by itself, and of
    every degree a wider bucket holds in that bucket."""
    got = _reached(described, codes, pack)
    want = set()
    for b in sc.BUCKET_ORDER:
        lo = {0: 3, 3: 9, 1: 11, 2: 17}[b]                       # natural bucket of the degrees from here on
        want |= {("CHK_CHAIN", d, b) for d in range(lo, sc.FUSED_CN_DEG[b] + 1)}
        want |= {("CHK_CHAIN", d, b) for d in range(3, min(lo, sc.FUSED_CN_DEG[b] + 1))}
    return want - got


@pytest.mark.parametrize("pack", [2, 1], ids=["nibble_rows", "byte_rows"])
def test_every_degree_is_decoded_on_every_path_that_holds_it(described, pack):
    """Variable degrees 1..20 and check degrees 2..32 under the per-class kernels; 1..kFusedVnDeg[b] and 2..kFusedCnDeg[b] under
    the fused kernel of every bucket b; the chained bodies of check degrees 3..32 likewise.  Exactly: nothing outside either."""
    assert not _sweep_gaps(described, SWEEP_CODES, pack)
    assert not _chain_gaps(described, list(sc.ZIGZAG), pack)
    degs = {(k, d) for k, d, _ in _reached(described, sc.CODES, pack)}
    assert {d for k, d in degs if k == "VAR"} == set(sc.VN_DEGREES) and {d for k, d in degs if k == "CHK"} == set(sc.CN_DEGREES)


def test_every_code_is_needed(described):
    """Without any one code of the tables the coverage above has a gap."""
    for name in SWEEP_CODES:
        assert _sweep_gaps(described, [n for n in SWEEP_CODES if n != name], 2), name
    for name in sc.ZIGZAG:
        assert _chain_gaps(described, [n for n in sc.ZIGZAG if n != name], 2), name


def test_every_case_is_on_the_path_it_names(described):
    """Bucket (the natural one, or widened by LUTLDPC_FUSED_BUCKET_MIN), skewed pipeline, row format, the specialised kernel names of
    every class."""
    for cid, (name, kn, desc) in described.items():
        sc.check_path(name, kn, desc)
        if name != sc.WIDE_LABELS and "LUTLDPC_SKEW" not in kn:
            assert desc["skewed_pipeline"] == 1, cid
    wide = described[sc.WIDE_LABELS + "-natural"][2]
    assert wide["pack"] == 1 and wide["skewed_pipeline"] == 0


def test_zigzag_runs_chain_every_check_class(described):
    """Every check class of a zigzag code holds nodes that are updated inside the check pass, about 3/4 of the checks in all (four
    checks per wave); none with LUTLDPC_CHAIN=0."""
    for cid, (name, kn, desc) in described.items():
        if name not in sc.ZIGZAG:
            assert desc["chain_nodes"] == 0 or 2 in sc.degrees(name)[0], cid
            continue
        per_class = [c["chain_nodes"] for c in desc["cn_classes"]]
        if "LUTLDPC_CHAIN" in kn:
            assert desc["chain_nodes"] == 0 and not any(per_class), cid
        else:
            assert all(n > 0 for n in per_class) and sum(per_class) == desc["chain_nodes"], (cid, per_class)
            assert all(c["nodes_per_wave"] >= 4 for c in desc["cn_classes"]), cid
            assert desc["chain_nodes"] >= 0.7 * sum(c["nodes"] for c in desc["cn_classes"]), cid


@pytest.mark.parametrize("name", sc.CODES)
def test_code_shapes(name, described):
    """At most kFusedMaxRoles degree classes, a positive rate, N of 500 to 1200; guests of 12 to 60 nodes beside the degree-3
    variables; no class size a multiple of 4 (the last block of a role is ragged) or of its nodes per wave (the last wave is)."""
    desc = described[name + "-natural"][2]
    cd = sc.codec(name)
    assert len(desc["vn_classes"]) + len(desc["cn_classes"]) <= sc.MAX_ROLES
    assert 500 <= cd.code.nvar <= 1200 and 0 < cd.code.nchk < cd.code.nvar
    if name in sc.SWEEP:
        assert all(12 <= n <= 60 for d, n in sc.SWEEP[name][0].items() if d != 3), name
    for c in desc["vn_classes"] + desc["cn_classes"]:
        assert c["nodes"] % 4 and (c["nodes_per_wave"] == 1 or c["nodes"] % c["nodes_per_wave"]), (name, c)


@pytest.mark.parametrize("cid,name,kn,n,quiet,want", sc.KNOB_CASES, ids=[c[0] for c in sc.KNOB_CASES])
def test_knob_case_shows_in_describe(cid, name, kn, n, quiet, want, monkeypatch):
    """The value of the case, and what the classes make of it: the nodes per wave in force."""
    dec, desc = sc.describe(name, kn, monkeypatch)
    dec.close()
    assert {k: desc[k] for k in want} == want, desc
    vn, cn = [c["nodes_per_wave"] for c in desc["vn_classes"]], [c["nodes_per_wave"] for c in desc["cn_classes"]]
    if "LUTLDPC_NODES_PER_WAVE" in kn:
        assert set(vn) == {want["nodes_per_wave"]}
    if "LUTLDPC_NODES_PER_WAVE" in kn or "LUTLDPC_NODES_PER_WAVE_CN" in kn:
        assert set(cn) == {want["nodes_per_wave_cn"]}            # (a fixed count also switches the widening of chain-rich classes off)
    if "LUTLDPC_VN_EDGES_PER_WAVE" in kn:
        assert set(vn) == {1}
    if "LUTLDPC_CN_EDGES_PER_WAVE" in kn:
        assert cn == [65536 // c["deg"] for c in desc["cn_classes"]]
    if "LUTLDPC_COMPACT" in kn:
        assert desc["compaction_min_groups"] == 4 and -(-n // desc["tile_frames"]) >= 4      # the batch reaches the check points


@pytest.mark.parametrize("name,n,snr", sc.CHK_FULL0, ids=[c[0] for c in sc.CHK_FULL0])
def test_chk_full_knob_shows_in_describe(name, n, snr, monkeypatch):
    from helpers import oracle_codec
    for value in ("1", "0"):
        dec, desc = sc.describe(name, dict(sc.STREAMING, LUTLDPC_CHK_FULL=value), monkeypatch, cd=oracle_codec(name))
        dec.close()
        assert desc["chk_full_labels"] == int(value)


@pytest.mark.parametrize("name", sc.CODES)
def test_batches_tell_decoders_apart(name):
    """With the oracle alone, on the batch every path decodes: at least 5 % of the frames converge, at least 5 % end without
    converging, the converged ones at two or more different iterations, and the planted frames pass on the channel decisions."""
    cd = sc.codec(name)
    cha, msg = sc.labels(name)
    cd.set_exit_conditions(cd.max_iters, True, True)
    _, it = cd.lut_decode_batch_flat(cha, msg)
    assert (it > 0).mean() >= 0.05 and (it < 0).mean() >= 0.05, ((it > 0).mean(), (it < 0).mean())
    assert len(set(it[it > 0].tolist())) >= 2 and (it == 0).sum() >= 3, sorted(set(it.tolist()))


@pytest.mark.parametrize("name", sc.KNOB_CODES)
def test_compaction_batch_empties_a_group_by_the_first_check_point(name):
    """The condition the compaction cases rely on: after the exit test of iteration 1 the active frames of either half (two groups)
    fit one group, and some frames are still active."""
    cd = sc.codec(name)
    cha, msg = sc.labels(name, sc.B_COMPACT, sc.COMPACT_QUIET)
    cd.set_exit_conditions(cd.max_iters, True, True)
    _, it = cd.lut_decode_batch_flat(cha, msg)
    active = (it < 0) | (it > 1)
    assert 0 < active[:1024].sum() <= 512 and 0 < active[1024:].sum() <= 512, (active[:1024].sum(), active[1024:].sum())


def test_a_code_may_have_any_number_of_degree_classes(monkeypatch):
    """Section E: 33 check classes on a host-only handle.  Degrees 2..32 run cn_minsum_fast_kernel, 33 and 34 the any-degree
    kernel; neither the fused pipeline nor the LDS-resident decoder takes the code, so every pass is per-class launches.  And the
    batch of the GPU test holds every iteration code from -5 to 5."""
    import numpy as np
    cd = sc.many_codec()
    dec, desc = sc.describe(None, {}, monkeypatch, cd=cd)
    dec.close()
    assert [c["deg"] for c in desc["cn_classes"]] == list(range(2, 35)) and [c["nodes"] for c in desc["cn_classes"]] == [3] * 33
    assert [c["kernel"] for c in desc["cn_classes"]] == ["cn_minsum_fast_kernel"] * 31 + ["cn_minsum_generic_kernel"] * 2, desc
    assert desc["resident"] == 0 and desc["skewed_pipeline"] == 0, desc
    cha, msg = sc.many_labels()
    cd.set_exit_conditions(cd.max_iters, True, True)
    _, it = cd.lut_decode_batch_flat(cha, msg)
    codes, counts = np.unique(it, return_counts=True)
    assert dict(zip(codes.tolist(), counts.tolist())) == sc.MANY_CODES


def test_describe_names_every_kernel_of_a_mixed_schedule(monkeypatch):
    """reg36_n1000_m16_12_8: the variable passes that write 12-label messages run the interpreter (no sign bit in a label of a
    12-label alphabet), the others the compile-time kernel; the check passes that read them likewise.  describe() names both,
    fast first."""
    from helpers import oracle_codec
    dec, desc = sc.describe(None, {}, monkeypatch, cd=oracle_codec("reg36_n1000_m16_12_8"))
    dec.close()
    assert [c["kernel"] for c in desc["vn_classes"]] == ["vn_balanced_fast_kernel+tree_pass_kernel<VAR>"], desc
    assert [c["kernel"] for c in desc["cn_classes"]] == ["cn_minsum_fast_kernel+cn_minsum_generic_kernel"], desc
