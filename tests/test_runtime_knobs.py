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
])
def test_knob_is_reflected_in_describe(clean_env, var, value, field, want):
    clean_env.setenv(var, value)
    assert _describe()[field] == want


def test_chain_fusion_switch(clean_env):
    assert _describe("dvbs2_q4_i6")["chain_nodes"] > 0
    clean_env.setenv("LUTLDPC_CHAIN", "0")
    assert _describe("dvbs2_q4_i6")["chain_nodes"] == 0
