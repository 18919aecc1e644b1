"""lutldpc_decoder_decode_llr_packed on the device: float64 / float32 / float16 / int8 soft values from host or device memory,
quantised straight into both row sets, a window of the decided bits out -- against the oracle's quant_nonlin of the widened values
and its decode of those labels (tests/llr_cases.py holds codes, values and references).  Everything is integer: equal bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import lut_ldpc_amd as L
from lut_ldpc_amd import _capi, packing
from lut_ldpc_amd._capi import ERR_ARG, LlrIO, check, last_error, lib

import llr_cases as lc
from helpers import CODES as CODE_DIR, PACKED_PATHS as PATHS, product_decoder
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

dp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
CODE = {"f64": _capi.LLR_F64, "f32": _capi.LLR_F32, "f16": _capi.LLR_F16, "i8": _capi.LLR_I8}
CANARY_W, CANARY_I, CANARY_L = 0xC0FFEE11, -12345, 0xA5


def quant_args(name, mode, q=None):
    qc, qm, mp = q or lc.quantiser(name)
    return dict(qb_cha=qc, qb_msg=qm if mode == 0 else None, cha2msg_map=mp if mode == 1 else None)


def dev(a):
    """A host array as a device tensor: a plain copy (none of torch's own kernels is needed), views are taken afterwards."""
    return torch.from_numpy(np.array(a)).to("cuda:0")


def to_host(*xs):
    return tuple(x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in xs)


def assert_window(words, it, want_bits, want_it, first, count, tag):
    words = words.view(np.uint32)
    assert words.shape == (len(want_it), (count + 31) // 32), tag
    assert (it == want_it).all(), (tag, np.flatnonzero(it != want_it)[:8])
    got = packing.unpack_bits(words, count)
    bad = np.argwhere(got != want_bits[:, first:first + count])
    assert bad.size == 0, (tag, f"{len(bad)} bit mismatches, first at frame/bit {bad[:4].tolist()}")
    if count % 32:                                           # bits beyond the window are 0
        assert (words[:, -1] >> np.uint32(count % 32) == 0).all(), tag


def assert_labels(cha, msg, want_cha, want_msg, tag):
    for got, want, what in ((cha, want_cha, "cha"), (msg, want_msg, "msg0")):
        bad = np.argwhere(got != want)
        assert bad.size == 0, (tag, what, f"{len(bad)} label mismatches, first at frame/node {bad[:4].tolist()}")


def run_parity(dec, name, B, dtypes=tuple(lc.DTYPES), device=False, tag=()):
    """Every exit mode x both modes x the dtypes: full window and labels, from host (or device) memory."""
    cd = lc.codec(name)
    N = cd.code.nvar
    for psc, pisc in lc.EXITS:
        dec.set_exit_conditions(cd.max_iters, psc, pisc)
        for mode in (0, 1):
            for dt in dtypes:
                x, scale, wide = lc.values(name, dt)
                wb, wi = lc.want(name, dt, mode, psc, pisc)
                wc, wm = lc.want_labels(name, dt, mode)
                lc.check_mix(name, wi[:B], pisc, B)
                src = dev(x[:B]) if device else x[:B]
                out = dec.decode_llr(src, scale=scale, want_labels=True, **quant_args(name, mode))
                if device:
                    assert all(isinstance(o, torch.Tensor) and o.is_cuda for o in out)
                words, it, cha, msg = to_host(*out)
                t = (name, B, dt, mode, psc, pisc, device) + tag
                assert_labels(cha, msg, wc[:B], wm[:B], t)
                assert_window(words, it, wb[:B], wi[:B], 0, N, t)
                if dt == "f64" and not device:                # the first-slice entry on the same handle and values
                    qc, qm, mp = lc.quantiser(name)
                    bits, it2 = dec.decode_llr_batch(x[:B], qc, qm, mode, mp if mode == 1 else None)
                    assert (it2 == wi[:B]).all() and (bits == wb[:B]).all(), t


@pytest.mark.parametrize("name,B", [(n, B) for n in lc.CASES for B in lc.batches(n)])
def test_llr_decode_matches_oracle_and_the_float64_entry(name, B):
    dec = product_decoder(lc.codec(name))
    desc = dec.describe()
    T = lc.CASES[name]["tile"]
    assert desc["tile_frames"] == T and desc["pack"] == (2 if T == 512 else 1), desc
    run_parity(dec, name, B)
    if B == T + 1:
        run_parity(dec, name, B, device=True)
    dec.close()


def spoiled(q):
    """Designed boundaries (15 or 31 here) with two adjacent entries swapped at a third of the array and the third from the end
    replaced by NaN."""
    q = q.copy()
    i = len(q) // 3
    q[[i, i + 1]] = q[[i + 1, i]]
    q[len(q) - 3] = np.nan
    return q


@pytest.mark.parametrize("name,B", [("n33", lc.CASES["n33"]["tile"] + 1), ("byte_q5", 257)])
def test_float64_entry_counts_the_leading_boundaries_of_any_array(name, B):
    """decode_llr_batch takes boundary arrays as its callers hold them: quant_nonlin stops at the first boundary that x does not
    exceed (the oracle's loop has the break), whatever comes after it -- a smaller boundary or NaN.  Every frame, bits and codes,
    against the oracle's decode of the oracle's labels; a map entry outside the message alphabet is refused."""
    cd = lc.codec(name)
    dec = product_decoder(cd)
    dec.set_exit_conditions(cd.max_iters, True, False)
    cd.set_exit_conditions(cd.max_iters, True, False)
    qc, qm, mp = lc.quantiser(name)
    sc, sm = spoiled(qc), spoiled(qm)
    x = lc.values(name, "f64")[0][:B]
    for mode in (0, 1):
        cha, msg = lc.ref_labels(x, sc, sm, mp, mode)
        assert (cha != lc.want_labels(name, "f64", mode)[0][:B]).any()          # the spoiled entries matter
        assert len(np.unique(cha)) < len(qc) + 1                               # ... labels behind them are out of reach
        wb, wi = cd.lut_decode_batch_flat(cha, msg)
        lc.check_mix(name, wi, False, B)
        bits, it = dec.decode_llr_batch(x, sc, sm if mode == 0 else None, mode, mp if mode == 1 else None)
        assert (it == wi).all(), (name, mode, np.flatnonzero(it != wi)[:8])
        assert (bits == wb).all(), (name, mode, np.argwhere(bits != wb)[:4].tolist())
    if name == "n33":
        bad = mp.copy()
        bad[len(bad) // 2] = len(qm) + 1                                       # = Nq_Msg[0]
        with pytest.raises(L.LutLdpcError, match="cha2msg_map entry outside") as e:
            dec.decode_llr_batch(x[:2], qc, None, 1, bad)
        assert e.value.code == ERR_ARG
        bits, it = dec.decode_llr_batch(x, sc, None, 1, mp)                    # the handle decodes as before
        assert (it == wi).all() and (bits == wb).all()
    dec.close()


@pytest.mark.parametrize("name", list(lc.CASES))
def test_windows_of_the_decided_bits(name):
    cd = lc.codec(name)
    dec = product_decoder(cd)
    N, K = cd.code.nvar, cd.code.nvar - cd.code.nchk
    B = lc.CASES[name]["tile"] + 1
    dec.set_exit_conditions(cd.max_iters, True, False)
    for k, (first, count) in enumerate(((0, K), (0, 1), (1, 32), (N - 33, 33))):
        mode, dt = k % 2, ("f32", "f16", "i8", "f64")[k]
        x, scale, _ = lc.values(name, dt)
        wb, wi = lc.want(name, dt, mode, True, False)
        words, it = dec.decode_llr(x[:B], scale=scale, first=first, count=count, **quant_args(name, mode))
        assert_window(words, it, wb[:B], wi[:B], first, count, (name, dt, mode, first, count))
    dec.close()


@pytest.mark.parametrize("bounds", ["designed", "awkward"])
def test_quantise_only_every_float16_pattern(bounds):
    name = "nib_q4"
    dec = product_decoder(lc.codec(name))
    N = 1000
    x = np.resize(np.arange(65536, dtype=np.uint16), 66 * N).view(np.float16).reshape(66, N)
    q = lc.quantiser(name) if bounds == "designed" else (lc.AWKWARD, np.sort(lc.AWKWARD * 0.75 + 0.01), lc.AWKWARD_MAP)
    for mode in (0, 1):
        wc, wm = lc.ref_labels(x.astype(np.float64), *q, mode)
        assert len(np.unique(wc)) > 8                        # (boundaries that round alike in float16 leave labels unused)
        for device in (False, True):
            out = dec.decode_llr(dev(x) if device else x, decode=False, **quant_args(name, mode, q))
            assert len(out) == 2
            cha, msg = to_host(*out)
            assert_labels(cha, msg, wc, wm, (bounds, mode, device))
    dec.close()


def raw_call(dec, name, dt, mode, B, src_ptr, stride, on_device, words, iters, cha, msg, first, count, scale):
    """The C-ABI itself: pointers as given (host arrays or device tensors), sync = 1."""
    qc, qm, mp = lc.quantiser(name)
    qc, qm, mp = np.ascontiguousarray(qc), np.ascontiguousarray(qm), np.ascontiguousarray(mp, np.int32)
    io = LlrIO(CODE[dt], int(on_device), stride, scale or 0.0, qc.ctypes.data_as(dp), len(qc), qm.ctypes.data_as(dp) if mode == 0 else None,
               len(qm) if mode == 0 else 0, mode, mp.ctypes.data_as(i32p) if mode == 1 else None, first, count, 1)
    ptr = lambda a: None if a is None else C.c_void_p(a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data)
    return lib.lutldpc_decoder_decode_llr_packed(dec._h, C.byref(io), C.c_void_p(src_ptr), B, ptr(words), ptr(iters), ptr(cha), ptr(msg))


@pytest.mark.parametrize("name,dt,B", [("nib_q4", "f32", 513), ("byte_q5", "f16", 257), ("n33", "i8", 511), ("n127", "f64", 40), ("n33", "f16", 513)])
def test_strides_bases_and_canaries(name, dt, B):
    """Frames N + 1 and N + 3 elements apart with poison in the gaps, a device base one element into an allocation; nothing is
    written after frame B - 1 of any output."""
    cd = lc.codec(name)
    dec = product_decoder(cd)
    dec.set_exit_conditions(cd.max_iters, True, True)
    N = cd.code.nvar
    x, scale, _ = lc.values(name, dt)
    T = lc.DTYPES[dt]
    poison = (np.nan, np.finfo(T).max) if dt != "i8" else (127, -128)
    first, count = 1, N - 1
    W = (count + 31) // 32
    k = 0
    for stride in (N + 1, N + 3):
        for on_device in (False, True):
            mode = k % 2
            wb, wi = lc.want(name, dt, mode, True, True)
            wc, wm = lc.want_labels(name, dt, mode)
            lead = 1 if on_device else 0                     # device: the base one element into the allocation
            flat = np.full(lead + B * stride, poison[k % 2], T)
            k += 1
            flat[lead:].reshape(B, stride)[:, :N] = x[:B]
            words = np.full((B + 3, W), CANARY_W, np.uint32)
            iters = np.full(B + 3, CANARY_I, np.int32)
            cha, msg = np.full((B + 3, N), CANARY_L, np.uint8), np.full((B + 3, N), CANARY_L, np.uint8)
            if on_device:
                src = dev(flat)
                words, iters, cha, msg = (dev(a.view(np.int32) if a.dtype == np.uint32 else a) for a in (words, iters, cha, msg))
                torch.cuda.synchronize()
                src_ptr = src.data_ptr() + flat.itemsize
            else:
                src_ptr = flat.ctypes.data
            check(raw_call(dec, name, dt, mode, B, src_ptr, stride, on_device, words, iters, cha, msg, first, count, scale))
            words, iters, cha, msg = to_host(words, iters, cha, msg)
            words = words.view(np.uint32)
            tag = (name, dt, B, stride, on_device)
            assert (words[B:] == CANARY_W).all() and (iters[B:] == CANARY_I).all() and (cha[B:] == CANARY_L).all() and (msg[B:] == CANARY_L).all(), tag
            assert_labels(cha[:B], msg[:B], wc[:B], wm[:B], tag)
            assert_window(words[:B], iters[:B], wb[:B], wi[:B], first, count, tag)
    dec.close()


@pytest.mark.parametrize("path", list(PATHS))
def test_every_decode_path_behind_the_llr_entry(path, monkeypatch):
    env, expect = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    name = "nib_q4"
    dec = product_decoder(lc.codec(name))
    desc = dec.describe()
    assert {k: desc[k] for k in expect} == expect, desc
    for rep in range(2):                                     # the second decode of a streaming path is the captured graph
        run_parity(dec, name, lc.CASES[name]["tile"] + 1, dtypes=("f32",), tag=(path, rep))
    dec.close()


def test_torch_tensors_in_torch_tensors_out():
    name = "nib_q4"
    cd = lc.codec(name)
    dec = product_decoder(cd)
    dec.set_exit_conditions(cd.max_iters, True, True)
    N, B = cd.code.nvar, 513
    for k, dt in enumerate(("f16", "f32")):
        mode = k % 2
        x, _, _ = lc.values(name, dt)
        host = dec.decode_llr(x[:B], want_labels=True, **quant_args(name, mode))
        wb, wi = lc.want(name, dt, mode, True, True)
        assert_window(host[0], host[1], wb[:B], wi[:B], 0, N, (dt, "host"))
        gaps = np.full((B, N + 3), np.nan, x.dtype)
        gaps[:, :N] = x[:B]
        wide = dev(gaps)
        for t in (dev(x[:B]), wide[:, :N]):
            out = dec.decode_llr(t, want_labels=True, **quant_args(name, mode))
            assert all(isinstance(o, torch.Tensor) and o.device == t.device for o in out)
            assert [o.dtype for o in out] == [torch.int32, torch.int32, torch.uint8, torch.uint8]
            for got, want in zip(to_host(*out), host):
                assert (got.view(want.dtype) == want).all(), (dt, t.stride())
        # a host tensor, one dimension, a transposed view (last dimension not contiguous), a wrong width
        for bad in (wide[:, :N].cpu(), wide[0, :N], dev(np.zeros((N, 4), x.dtype)).t(), wide[:, :N - 1], wide):
            with pytest.raises(ValueError):
                dec.decode_llr(bad, **quant_args(name, mode))
    dec.close()


def test_codec_decode_llr_returns_the_data_bits():
    """Codec.decode_llr: boundaries, mode, map and K from the codec, against the codec's own byte entry."""
    pcd = L.Codec(CODE_DIR / "rate0.50_dv02-17_dc08-09_lut_q4_N500.alist", device=0)
    pcd.design_luts(sigma2=0.88 ** 2, max_iters=8)
    pcd.set_exit_conditions(8, True, True)
    rng = np.random.default_rng(57)
    N0 = 10 ** (-2.0 / 10) / pcd.rate
    llr = 4 * (1.0 + rng.normal(0.0, np.sqrt(N0 / 2), (600, pcd.nvar))) / N0
    K = pcd.ninfo
    for mode in (0, 1):
        pcd.set_initial_message_mode(mode)
        for T in (np.float64, np.float32, np.float16):
            x = llr.astype(T)
            cha = orc.quant_nonlin(x.astype(np.float64), pcd.qb_cha)
            msg = orc.quant_nonlin(x.astype(np.float64), pcd.qb_msg) if mode == 0 else pcd.cha2msg_map[cha].astype(np.uint8)
            bits, it = pcd.lut_decode_batch(cha, msg)
            assert (it > 0).any() and (it < 0).any()
            words, got_it = pcd.decode_llr(x)
            assert words.shape == (600, (K + 31) // 32) and (got_it == it).all()
            assert (packing.unpack_bits(words, K) == bits[:, :K]).all()
            words, got_it = pcd.decode_llr(dev(x), info_only=False)
            words, got_it = to_host(words, got_it)
            assert (packing.unpack_bits(words.view(np.uint32), pcd.nvar) == bits).all() and (got_it == it).all()
    pcd.close()


def test_argument_errors_on_a_device_handle():
    name = "nib_q4"
    cd = lc.codec(name)
    dec = product_decoder(cd)
    N, B = cd.code.nvar, 5
    x, _, _ = lc.values(name, "f32")
    xi, scale, _ = lc.values(name, "i8")
    qc, qm, mp = lc.quantiser(name)
    words, iters = np.zeros((B, 32), np.uint32), np.zeros(B, np.int32)
    buf = np.zeros(B * N + 1, np.float32)

    def refused(rc, text):
        assert rc == ERR_ARG and text in last_error(), (rc, last_error())

    refused(raw_call(dec, name, "f32", 0, B, buf.ctypes.data + 2, N, False, words, iters, None, None, 0, N, None), "aligned")
    refused(raw_call(dec, name, "f32", 0, B, buf.ctypes.data, N - 1, False, words, iters, None, None, 0, N, None), "frame_stride")
    refused(raw_call(dec, name, "i8", 1, B, xi.ctypes.data, N, False, words, iters, None, None, 0, N, -scale), "scale")
    refused(raw_call(dec, name, "i8", 1, B, xi.ctypes.data, N, False, words, iters, None, None, 0, N, float("inf")), "scale")
    with pytest.raises(L.LutLdpcError, match="non-decreasing"):
        dec.decode_llr(x[:B], qc[::-1].copy(), qb_msg=qm)
    with pytest.raises(L.LutLdpcError, match="non-decreasing"):
        dec.decode_llr(dev(x[:B]), qc, qb_msg=qm[::-1].copy())
    # the handle decodes as before
    dec.set_exit_conditions(cd.max_iters, True, False)
    wb, wi = lc.want(name, "f32", 0, True, False)
    out = dec.decode_llr(x[:B], **quant_args(name, 0))
    assert_window(out[0], out[1], wb[:B], wi[:B], 0, N, "after the refusals")
    dec.close()
