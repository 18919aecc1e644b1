"""The run-time knobs (environment variables read once, at decoder creation, through the table in decoder.hip) as describe()
reports them on host-only handles: no GPU needed.  monkeypatch restores the environment."""
import pytest

from helpers import oracle_codec, product_decoder


def _describe(name="n500_q4"):
    dec = product_decoder(oracle_codec(name), device=-1)
    desc = dec.describe()
    dec.close()
    return desc


@pytest.fixture
def clean_env(monkeypatch):
    import os
    for k in [k for k in os.environ if k.startswith("LUTLDPC_") and k not in ("LUTLDPC_LIB", "LUTLDPC_DESIGN_CACHE")]:
        monkeypatch.delenv(k)
    return monkeypatch


def test_defaults(clean_env):
    d = _describe()
    assert d["pack"] == 2 and d["message_bytes"] == 0.5
    assert d["use_fast"] == 1 and d["skewed_pipeline"] == 1
    assert d["compaction"] == 2                                   # automatic
    assert d["vn_edges_per_wave"] == 16 and d["cn_edges_per_wave"] == 42 and d["nodes_per_block"] == 16
    assert d["resident"] == 0                                     # never on a host-only handle
    assert d["nodes_per_wave"] == 0 and d["nodes_per_wave_cn"] == 0      # unset: derived per class from the edges per wave
    assert d["tail_front"] == 0.25 and d["fused_prio"] == 0 and d["chk_full_labels"] == 1
    assert [(c["deg"], c["nodes_per_wave"]) for c in d["vn_classes"]] == [(2, 8), (3, 5), (9, 1), (17, 1)]
    assert [(c["deg"], c["nodes_per_wave"], c["chain_nodes"]) for c in d["cn_classes"]] == [(8, 5, 0), (9, 4, 0), (10, 4, 0)]


@pytest.mark.parametrize("var,value,field,want", [
    ("LUTLDPC_PACK", "1", "pack", 1),
    ("LUTLDPC_PACK", "1", "message_bytes", 1),
    ("LUTLDPC_PACK", "2", "pack", 2),                             # only 1 is accepted
    ("LUTLDPC_USE_FAST", "0", "use_fast", 0),
    ("LUTLDPC_USE_FAST", "0", "skewed_pipeline", 0),              # the fused pipeline needs the specialised kernels
    ("LUTLDPC_COMPACT", "1", "compaction", 1),
    ("LUTLDPC_COMPACT", "0", "compaction", 0),
    ("LUTLDPC_SKEW", "0", "skewed_pipeline", 0),
    ("LUTLDPC_VN_EDGES_PER_WAVE", "32", "vn_edges_per_wave", 32),
    ("LUTLDPC_VN_EDGES_PER_WAVE", "0", "vn_edges_per_wave", 16),  # outside the range: ignored, not clamped
    ("LUTLDPC_VN_EDGES_PER_WAVE", "65537", "vn_edges_per_wave", 16),
    ("LUTLDPC_CN_EDGES_PER_WAVE", "24", "cn_edges_per_wave", 24),
    ("LUTLDPC_NODES_PER_BLOCK", "8", "nodes_per_block", 8),
    ("LUTLDPC_NODES_PER_BLOCK", "5000", "nodes_per_block", 16),
    ("LUTLDPC_NODES_PER_WAVE", "3", "nodes_per_wave", 3),
    ("LUTLDPC_NODES_PER_WAVE", "3", "nodes_per_wave_cn", 3),         # the check side follows unless it has a value of its own
    ("LUTLDPC_NODES_PER_WAVE", "4097", "nodes_per_wave", 0),
    ("LUTLDPC_NODES_PER_WAVE_CN", "2", "nodes_per_wave_cn", 2),
    ("LUTLDPC_NODES_PER_WAVE_CN", "2", "nodes_per_wave", 0),
    ("LUTLDPC_TAIL_FRONT", "0", "tail_front", 0),
    ("LUTLDPC_TAIL_FRONT", "0.89", "tail_front", 0.89),
    ("LUTLDPC_TAIL_FRONT", "0.9", "tail_front", 0.25),               # the upper limit is exclusive
    ("LUTLDPC_PRIO", "1", "fused_prio", 1),
    ("LUTLDPC_CHK_FULL", "0", "chk_full_labels", 0),
])
def test_knob_is_reflected_in_describe(clean_env, var, value, field, want):
    clean_env.setenv(var, value)
    assert _describe()[field] == want


def test_nodes_per_wave_in_force(clean_env):
    """The classes report what the knobs make of them: a fixed count on both sides, on the check side alone, from the edges per wave."""
    clean_env.setenv("LUTLDPC_NODES_PER_WAVE", "3")
    d = _describe()
    assert {c["nodes_per_wave"] for c in d["vn_classes"] + d["cn_classes"]} == {3}
    clean_env.setenv("LUTLDPC_NODES_PER_WAVE_CN", "2")
    d = _describe()
    assert {c["nodes_per_wave"] for c in d["vn_classes"]} == {3} and {c["nodes_per_wave"] for c in d["cn_classes"]} == {2}
    clean_env.delenv("LUTLDPC_NODES_PER_WAVE")
    clean_env.delenv("LUTLDPC_NODES_PER_WAVE_CN")
    clean_env.setenv("LUTLDPC_CN_EDGES_PER_WAVE", "24")
    assert [c["nodes_per_wave"] for c in _describe()["cn_classes"]] == [3, 2, 2]


def test_chain_fusion_switch(clean_env):
    """DVB-S2: the one chain-rich class (degree 7, the zigzag) runs twelve checks per wave and holds every chained node."""
    d = _describe("dvbs2_q4_i6")
    assert d["chain_nodes"] > 0 and sum(c["chain_nodes"] for c in d["cn_classes"]) == d["chain_nodes"]
    rich = max(d["cn_classes"], key=lambda c: c["chain_nodes"])
    assert rich["nodes_per_wave"] == 12 and rich["chain_nodes"] >= 0.9 * rich["nodes"], rich
    clean_env.setenv("LUTLDPC_CHAIN", "0")
    d = _describe("dvbs2_q4_i6")
    assert d["chain_nodes"] == 0 and not any(c["chain_nodes"] for c in d["cn_classes"])
    assert all(c["nodes_per_wave"] == 42 // c["deg"] for c in d["cn_classes"])


def test_removed_knobs_change_nothing(clean_env):
    """LUTLDPC_COMPOSE, LUTLDPC_COMPOSE_SPACE and LUTLDPC_COMPACT_KEEP selected variants that measured slower and are gone with
    their code: setting them leaves describe() and the generated resident sources as a clean environment gives them."""
    def snapshot():
        out = [_describe("n500_q4")]
        for name, G in (("reg36_n1000_mixed", 1), ("c5_chklut", 2)):
            dec = product_decoder(oracle_codec(name), device=-1)
            out.append(dec.resident_source(G))
            dec.close()
        return out

    clean = snapshot()
    for k, v in (("LUTLDPC_COMPOSE", "1"), ("LUTLDPC_COMPOSE_SPACE", "64"), ("LUTLDPC_COMPACT_KEEP", "0")):
        clean_env.setenv(k, v)
    assert snapshot() == clean
