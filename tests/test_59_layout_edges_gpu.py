"""The frame-major <-> row kernels (kernels_layout.hpp) at the shapes where they can go wrong, through the byte entries that use
them: labels in (labels_in_kernel, byte input, one row set) and labels out (transpose_out_kernel), each in its dword form (frame
size a multiple of 4 and a 4-byte aligned buffer) and in its byte form (anything else).

Codes: the two odd-N codes of frontend_cases.py (N = 33: a single node block, last quad one node; N = 127: last quad three nodes;
both take the byte forms whatever the buffer) and reg36_n1000_q4 (N = 1000 = 7 x 128 + 104: dword forms from aligned buffers, byte
forms from buffers that start one byte later), in nibble rows and, through the `_pack1` handles, in byte rows.  Batches 1, tile - 1
and tile + 1 frames: prefixes of one batch per code whose even frames are sampled at a high and whose odd frames at a low SNR, with
labels above the alphabet planted in both arrays (the kernels clamp them: the expected result is the oracle's on the clamped labels).

The LDS-resident decoder reads and writes the caller's frame-major arrays itself, so every handle here is made with
LUTLDPC_RESIDENT=0: the streaming decode, which goes through the row layout.  Everything is integer: equal bit for bit."""
import functools

import numpy as np
import pytest

import frontend_cases as fc
from helpers import awgn_labels, product_decoder
from stats_helpers import parse_dump_text

pytestmark = pytest.mark.gpu

HANDLES = ("n33", "n127", "n127_pack1", "q4", "q4_pack1")
SNR = {"n33": (1.0, 5.0), "n127": (1.0, 5.0), "reg36_n1000_q4": (1.0, 3.0)}      # (odd, even frames), dB
T_MAX = 512
CANARY = 0xA5


@functools.lru_cache(maxsize=None)
def labels(code):
    """T_MAX + 1 frames: (cha, msg) as sent, with labels above the alphabets, and the oracle's (bits, iters) on the clamped ones."""
    cd = fc.codec(code)
    lo, hi = SNR[code]
    a, b = awgn_labels(cd, T_MAX + 1, hi, seed=5900), awgn_labels(cd, T_MAX + 1, lo, seed=5901)
    cha, msg = a[0].copy(), a[1].copy()
    cha[1::2], msg[1::2] = b[0][1::2], b[1][1::2]
    rng = np.random.default_rng(59)
    sent = []
    for x, nq in ((cha, cd.nq_cha), (msg, int(cd.nq_msg[0]))):
        hit = rng.random(x.shape) < 0.05
        x[hit] = nq - 1
        s = x.copy()
        s[hit] = rng.integers(nq, 256, int(hit.sum()))
        assert hit[0].any() and s.max() > 200
        sent.append(s)
    cd.set_exit_conditions(cd.max_iters, True, True)
    bits, it = cd.lut_decode_batch_flat(cha, msg)
    assert (it > 0).any() and (it < 0).any()
    for x in (*sent, bits, it):
        x.setflags(write=False)
    return sent[0], sent[1], bits, it


def decoder_of(handle, monkeypatch):
    code, env, T = fc.HANDLES[handle]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("LUTLDPC_RESIDENT", "0")
    cd = fc.codec(code)
    dec = product_decoder(cd)
    desc = dec.describe()
    assert desc["resident"] == 0 and desc["tile_frames"] == T, desc
    return code, cd, dec, T


def on_device(arr, lead):
    """`arr` in device memory `lead` bytes behind a 4-byte aligned address (filled on the host: copies only)."""
    import torch
    flat = np.concatenate([np.full(lead, CANARY, np.uint8), arr.reshape(-1)])
    t = torch.from_numpy(flat).to(torch.device("cuda", 0))
    assert t.data_ptr() % 4 == 0
    return t, t[lead:]


@pytest.mark.parametrize("handle,bk", [(h, bk) for h in HANDLES for bk in ("1", "T-1", "T+1")])
def test_byte_entries_from_host_aligned_and_offset_device_buffers(handle, bk, monkeypatch):
    import torch
    code, cd, dec, T = decoder_of(handle, monkeypatch)
    B, N = fc.batch_size(bk, T), cd.code.nvar
    cha, msg, want_bits, want_it = (x[:B] for x in labels(code))
    dec.set_exit_conditions(cd.max_iters, True, True)
    # 1. the host entry
    bits, it = dec.lut_decode_batch(cha, msg)
    assert (it == want_it).all(), (handle, B, np.flatnonzero(it != want_it)[:8])
    assert (bits == want_bits).all(), (handle, B, np.argwhere(bits != want_bits)[:4].tolist())
    # 2. the device entry on aligned buffers, 3. on buffers one byte behind an aligned address
    for lead in (0, 1):
        keep = [on_device(cha, lead), on_device(msg, lead)]
        out, out_v = on_device(np.full((B + 1, N), CANARY, np.uint8), lead)
        its = torch.from_numpy(np.full(B + 4, -77, np.int32)).to(out.device)
        assert out_v.data_ptr() % 4 == lead and keep[0][1].data_ptr() % 4 == lead
        dec.lut_decode_batch_device(keep[0][1].data_ptr(), keep[1][1].data_ptr(), B, out_v.data_ptr(), its.data_ptr(), sync=True)
        got, got_it = out.cpu().numpy(), its.cpu().numpy()
        assert (got_it[:B] == it).all() and (got_it[B:] == -77).all(), (handle, B, lead)
        assert (got[lead:lead + B * N].reshape(B, N) == bits).all(), (handle, B, lead)
        assert (got[:lead] == CANARY).all() and (got[lead + B * N:] == CANARY).all(), (handle, B, lead)      # before frame 0, frame B
        for (t, _), sent in zip(keep, (cha, msg)):
            assert (t.cpu().numpy()[lead:] == sent.reshape(-1)).all()
    dec.close()


@pytest.mark.parametrize("handle", ["n33", "n127", "n127_pack1"])
def test_message_trace_of_an_edge_count_that_is_no_multiple_of_four(handle, monkeypatch):
    """transpose_out_kernel over E rows (n33: 66, n127: 381): dump 0 is every edge's initial message, and every dump of every frame
    is what the oracle prints for it (output_verbosity 3, exit tests off)."""
    code, cd, dec, T = decoder_of(handle, monkeypatch)
    E, I, B = cd.code.nedges, cd.max_iters, 9
    assert E % 4
    cha, msg = (np.minimum(x[:B], nq - 1) for x, nq in zip(labels(code)[:2], (cd.nq_cha, int(cd.nq_msg[0]))))
    cd.set_exit_conditions(I, False, False)
    dec.set_exit_conditions(I, False, False)
    want_bits, want_it, txt = cd.lut_decode_dump(cha, msg, 3)
    printed = parse_dump_text(txt, E)
    bits, it, tr = dec.lut_decode_batch_trace(cha, msg, 3, E)
    assert tr.shape == (1 + 2 * I, B, E) and (it == want_it).all() and (bits == want_bits).all()
    assert (tr[0] == np.repeat(msg, cd.code.dv, axis=1)).all()
    assert len(printed) == B
    for f, dumps in enumerate(printed):
        assert dumps.shape == (1 + 2 * I, E) and (tr[:, f] == dumps).all(), (handle, f, np.argwhere(tr[:, f] != dumps)[:4].tolist())
    dec.close()
