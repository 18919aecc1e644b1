"""Every degree of the streaming pass kernels against the oracle.  pass_fused_kernel, cn_minsum_fast_kernel and
vn_balanced_fast_kernel are some 250 instantiations whose code the degree decides at compile time; the other tests decode a dozen
of those degrees.  The codes of tests/streaming_cases.py hold every variable degree 1..20 and every check degree 2..32 in ragged
classes (section A), and every check degree 3..32 chained along a zigzag (section B); each code runs through its own bucket of the
fused kernel in nibble and in byte rows, every wider bucket, the per-class kernels, a single partly filled frame group, and the
edge-initialising first pass (section C); two of them through the work-partitioning and scheduling knobs no other test sets
(section D).  Every case first asserts from describe() that it is on the path it names, then decodes bit-exact against the oracle
in the three exit modes; the oracle decodes a batch once per mode for all paths.  tests/test_streaming_cases_cpu.py computes what
these cases cover and checks that their batches tell decoders apart."""
import pytest

import streaming_cases as sc
from helpers import awgn_labels, compare, oracle_codec

pytestmark = pytest.mark.gpu


def _decode(dec, cd, cha, msg, cache):
    """All three exit modes against the (shared) oracle result; returns the iteration codes with both exit tests on."""
    its = [compare(cd, dec, cha, msg, psc, pisc, flat=True, cache=cache) for psc, pisc in sc.EXIT_MODES]
    return its[0]


@pytest.mark.parametrize("cid,name,kn,n", sc.CASES, ids=[c[0] for c in sc.CASES])
def test_degree_sweep(cid, name, kn, n, monkeypatch):
    """Sections A to C: one (code, path).  The first n frames of the code's batch: the planted frames pass on the channel decisions,
    the others converge at several iterations or not at all (checked on the CPU for the whole batch)."""
    dec, desc = sc.describe(name, kn, monkeypatch, device=0)
    sc.check_path(name, kn, desc)
    if name in sc.ZIGZAG:
        assert all((c["chain_nodes"] > 0) == ("LUTLDPC_CHAIN" not in kn) for c in desc["cn_classes"]), desc
    cha, msg = sc.labels(name, n)
    it = _decode(dec, sc.codec(name), cha, msg, sc.oracle_cache(name))
    assert (it == 0).sum() >= 3 and (it > 0).any() and (it < 0).any()
    dec.close()


@pytest.mark.parametrize("cid,name,kn,n,quiet,want", sc.KNOB_CASES, ids=[c[0] for c in sc.KNOB_CASES])
def test_knobs(cid, name, kn, n, quiet, want, monkeypatch):
    """Section D: nodes and edges per wave from one node to the whole class, the tail of the fused launches, the issue priority, the
    interpreter kernels' nodes per block, compaction weighing cost against gain -- each shown by describe() before the decode."""
    dec, desc = sc.describe(name, kn, monkeypatch, device=0)
    sc.check_path(name, kn, desc)
    assert {k: desc[k] for k in want} == want, desc
    cha, msg = sc.labels(name, n, quiet)
    it = _decode(dec, sc.codec(name), cha, msg, sc.oracle_cache(name))
    assert (it == 0).sum() >= 3 and (it > 0).any() and (it < 0).any()
    dec.close()


@pytest.mark.parametrize("name,n,snr", sc.CHK_FULL0, ids=[c[0] for c in sc.CHK_FULL0])
def test_generated_check_kernels_on_sign_magnitude_tables(name, n, snr, monkeypatch):
    """LUTLDPC_CHK_FULL=0: the generated CHKTREE kernels walk (sign, magnitude) tables as the reference does, instead of the
    full-label tables the default builds."""
    cd = oracle_codec(name)
    dec, desc = sc.describe(name, dict(sc.STREAMING, LUTLDPC_CHK_FULL="0"), monkeypatch, device=0, cd=cd)
    assert desc["chk_full_labels"] == 0 and desc["resident"] == 0 and {c["kernel"] for c in desc["cn_classes"]} == {"lutldpc_jit_pass"}, desc
    cha, msg, _ = awgn_labels(cd, n, snr, seed=n, mode=1 if name.startswith("c5") else 0)
    it = _decode(dec, cd, cha, msg, None)
    assert len(set(it.tolist())) >= 3
    dec.close()


def test_more_degree_classes_than_one_interpreter_launch_once_held(monkeypatch):
    """Section E of streaming_cases.py: 33 check classes.  With no knob the check pass is 31 launches of cn_minsum_fast_kernel and two
    of cn_minsum_generic_kernel (degrees 33, 34); with LUTLDPC_USE_FAST=0 every class of both passes runs the interpreter."""
    import numpy as np
    cd = sc.many_codec()
    cha, msg = sc.many_labels()
    cache = {}
    for kn in ({}, {"LUTLDPC_USE_FAST": "0"}):
        dec, desc = sc.describe(None, kn, monkeypatch, device=0, cd=cd)
        assert desc["resident"] == 0 and desc["skewed_pipeline"] == 0 and len(desc["cn_classes"]) == 33, desc
        generic = ["cn_minsum_generic_kernel"] * 33 if kn else ["cn_minsum_fast_kernel"] * 31 + ["cn_minsum_generic_kernel"] * 2
        assert [c["kernel"] for c in desc["cn_classes"]] == generic, desc
        assert desc["vn_classes"][0]["kernel"] == ("tree_pass_kernel<VAR>" if kn else "vn_balanced_fast_kernel"), desc
        it = _decode(dec, cd, cha, msg, cache)
        codes, counts = np.unique(it, return_counts=True)
        assert dict(zip(codes.tolist(), counts.tolist())) == sc.MANY_CODES
        dec.close()
