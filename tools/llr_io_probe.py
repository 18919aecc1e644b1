#!/usr/bin/env python3
"""What it costs to decode soft values as a receiver holds them, and what lutldpc_decoder_decode_llr_packed saves over the
first-slice entry lutldpc_decoder_decode_llr_batch (float64 from host memory, a byte per decided bit back).
Per workload (DVB-S2 at 8192 frames: the float64 batch is 4.2 GB; the (3,6) N = 10000 code at 4096), in ONE process, as-shipped
exit conditions (psc and pisc), 0.4 dB above the design point, initial messages = cha2msg_map of the channel labels (QCHA):
  llr_batch     lutldpc_decoder_decode_llr_batch on float64, a byte per decided bit back (the same quantiser as the rows below)
  host f64 .. host i8   the new entry on host float64 / float32 / float16 / int8 (scale = 1.25 max|qb| / 127), data bits out
  dev f32, dev f16      the new entry on tensors that already live in HBM, data bits left there
  device        lutldpc_decoder_decode_batch_device on label buffers in HBM: no transfer, no quantiser -- the ceiling
The values are float32 numbers (made in HBM by torch's Philox normal generator), so float64 and float32 carry the same values;
float16 and int8 are roundings of them and decode to their own results.  Wall time per batch from a host clock around calls that
end in a stream synchronise; all buffers exist and are touched before the first call; 2 warm-up rounds, then 5 timed rounds with
the entries alternating; median, min and max.  Results are compared: host f64 and f32 with llr_batch, dev with host, on every frame.
Then the label kernel alone, from the library's profile (LUTLDPC_K_LAYOUT) of quantise-only calls on the device tensor: a call that
returns one label array runs the label kernel and one transpose out, a call that returns both runs two, so
label kernel = 2 x (one) - (both); next to it a device-to-device copy of as many bytes as the kernel moves (input + both row sets).
One JSON line per workload after the table.
Usage: tools/llr_io_probe.py [--rounds 5] [--warmup 2] [--frames B] [workload ...]      (default: dvbs2 c2)"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np

import bench
import lut_ldpc_amd as L
from lut_ldpc_amd import packing

FRAMES = {"dvbs2": 8192, "c2": 4096}


def run(wl, rounds, warmup, frames):
    import torch
    alist, sigma, max_iter, qc, qm, B, extra, known_rank = bench.WORKLOADS[wl]
    B = frames or FRAMES.get(wl, B)
    cd = L.Codec(ROOT / "data" / "codes" / f"{alist}.alist", known_rank=known_rank, device=0)
    cd.design_luts(sigma2=sigma * sigma, max_iters=max_iter, nq_cha=1 << qc, nq_msg=1 << qm, **extra)
    cd.set_initial_message_mode(1)
    cd.set_exit_conditions(max_iter, True, True)
    dec = cd.decoder()
    N, K = cd.nvar, cd.ninfo
    snr = -10 * np.log10(2 * cd.rate * sigma * sigma) + 0.4
    qb, mp = cd.qb_cha, np.ascontiguousarray(cd.cha2msg_map, np.int32)
    scale = float(np.float32(1.25 * np.abs(qb).max() / 127.0))
    N0 = 10 ** (-snr / 10) / cd.rate
    g = torch.Generator(device="cuda")
    g.manual_seed(57)
    d32 = torch.empty((B, N), dtype=torch.float32, device="cuda")
    step = max(1, (1 << 27) // N)
    for b0 in range(0, B, step):
        n = min(step, B - b0)
        d32[b0:b0 + n] = (1.0 + torch.randn((n, N), generator=g, device="cuda", dtype=torch.float32) * float(np.sqrt(N0 / 2))) * (4.0 / N0)
    d16 = d32.to(torch.float16)
    h = {"f32": d32.cpu().numpy(), "f16": d16.cpu().numpy(), "i8": torch.clamp(torch.round(d32 / scale), -128, 127).to(torch.int8).cpu().numpy()}
    h["f64"] = h["f32"].astype(np.float64)
    torch.cuda.synchronize()
    kw = dict(qb_cha=qb, cha2msg_map=mp, first=0, count=K)
    # label buffers for the ceiling: what the device derives from the float32 tensor
    d_cha, d_msg = dec.decode_llr(d32, decode=False, **kw)
    d_bits = torch.zeros((B, N), dtype=torch.uint8, device="cuda")
    d_its = torch.zeros(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    res = {}

    def keep(name, f):
        def call():
            res[name] = f()
        return call

    W = (K + 31) // 32
    esize = {"f64": 8, "f32": 4, "f16": 2, "i8": 1}
    entries = {"llr_batch": keep("llr_batch", lambda: dec.decode_llr_batch(h["f64"], qb, None, 1, mp))}
    moved = {"llr_batch": (8 * B * N, B * N + 4 * B), "device": (0, 0)}
    for dt in ("f64", "f32", "f16", "i8"):
        entries["host " + dt] = keep("host " + dt, lambda dt=dt: dec.decode_llr(h[dt], scale=scale if dt == "i8" else None, **kw))
        moved["host " + dt] = (esize[dt] * B * N, 4 * B * W + 4 * B)
    for dt, t in (("f32", d32), ("f16", d16)):
        entries["dev " + dt] = keep("dev " + dt, lambda t=t: dec.decode_llr(t, **kw))
        moved["dev " + dt] = (0, 0)
    entries["device"] = lambda: dec.lut_decode_batch_device(d_cha.data_ptr(), d_msg.data_ptr(), B, d_bits.data_ptr(), d_its.data_ptr(), sync=True)
    ms = {k: [] for k in entries}
    for r in range(warmup + rounds):
        for k, call in entries.items():
            t0 = time.perf_counter()
            call()
            dt_ms = (time.perf_counter() - t0) * 1e3
            if r >= warmup:
                ms[k].append(dt_ms)
    bits, its = res["llr_batch"]
    data = lambda words: packing.unpack_bits(np.ascontiguousarray(words).view(np.uint32), K)
    same = {k: bool((res[k][1] == its).all() and (data(res[k][0]) == bits[:, :K]).all()) for k in ("host f64", "host f32")}
    for dt in ("f32", "f16"):
        w, i = (x.cpu().numpy() for x in res["dev " + dt])
        same["dev " + dt] = bool((i == res["host " + dt][1]).all() and (w.view(np.uint32) == res["host " + dt][0]).all())
    same["device"] = bool((d_its.cpu().numpy() == its).all() and (d_bits.cpu().numpy()[:, :K] == bits[:, :K]).all())
    out = {"workload": wl, "B": B, "nvar": N, "K_info": K, "snr_db": round(float(snr), 3), "rounds": rounds, "warmup": warmup, "equal": same,
           "converged": int((its >= 0).sum()), "failed": int((its < 0).sum())}
    print(f"{wl}: {B} frames, N = {N}, K = {K}, {snr:.2f} dB, {out['converged']} frames converged, {out['failed']} failed; results equal: {same}")
    print(f"  {'entry':10s} {'MB in':>9s} {'MB out':>9s} {'median ms':>10s} {'min ms':>9s} {'max ms':>9s} {'frames/s':>10s}")
    for k in entries:
        med = float(np.median(ms[k]))
        out[k] = {"bytes_in": moved[k][0], "bytes_out": moved[k][1], "ms_median": round(med, 2), "ms_min": round(min(ms[k]), 2), "ms_max": round(max(ms[k]), 2)}
        print(f"  {k:10s} {moved[k][0] / 1e6:9.1f} {moved[k][1] / 1e6:9.1f} {med:10.2f} {min(ms[k]):9.2f} {max(ms[k]):9.2f} {B / med * 1e3:10.0f}")
    for k in ("host f64", "host f32", "host f16", "host i8", "dev f32", "dev f16", "device"):
        out[k.replace(" ", "_") + "_over_llr_batch_time"] = round(out[k]["ms_median"] / out["llr_batch"]["ms_median"], 3)
    # the label kernel alone
    tile = dec.describe()["tile_frames"]
    rows = 2 * ((B + tile - 1) // tile) * N * 256
    print(f"  {'label kernel':14s} {'MB moved':>9s} {'kernel ms':>10s} {'GB/s':>8s} {'copy ms':>9s} {'copy GB/s':>10s}")
    dec.set_profiling(True)
    for dt, t in (("f32", d32), ("f16", d16)):
        lay = []
        for both in (False, True):
            io_kw = dict(qb_cha=qb, cha2msg_map=mp)
            per = []
            for r in range(warmup + rounds):
                dec.reset_profile()
                if both:
                    dec.decode_llr(t, decode=False, **io_kw)
                else:
                    one_label(dec, t, qb, mp, d_cha)
                if r >= warmup:
                    per.append(dec.profile()["layout"]["ms"])
            lay.append(float(np.median(per)))
        k_ms = 2 * lay[0] - lay[1]
        nbytes = esize[dt] * B * N + rows
        a = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        b = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        cp = []
        for r in range(warmup + rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            b.copy_(a)
            e1.record()
            e1.synchronize()
            if r >= warmup:
                cp.append(e0.elapsed_time(e1))
        c_ms = float(np.median(cp))
        del a, b
        out["label_kernel_" + dt] = {"bytes": nbytes, "layout_ms_one_label": round(lay[0], 3), "layout_ms_both_labels": round(lay[1], 3), "kernel_ms": round(k_ms, 3),
                                     "copy_ms": round(c_ms, 3)}
        print(f"  {dt:14s} {nbytes / 1e6:9.1f} {k_ms:10.3f} {nbytes / k_ms / 1e6:8.0f} {c_ms:9.3f} {2 * nbytes / c_ms / 1e6:10.0f}   (copy: read + write)")
    dec.set_profiling(False)
    print(json.dumps(out), flush=True)
    cd.close()
    return all(same.values())


def one_label(dec, t, qb, mp, d_cha):
    """Quantise only, the channel labels alone returned (Decoder.decode_llr always asks for both)."""
    from lut_ldpc_amd import _capi
    dp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    codes = {2: _capi.LLR_F16, 4: _capi.LLR_F32}
    qb = np.ascontiguousarray(qb, np.float64)
    io = _capi.LlrIO(codes[t.element_size()], 1, t.stride(0), 0.0, qb.ctypes.data_as(dp), len(qb), None, 0, 1, mp.ctypes.data_as(i32p), 0, 1, 1)
    _capi.check(_capi.lib.lutldpc_decoder_decode_llr_packed(dec._h, C.byref(io), C.c_void_p(t.data_ptr()), t.shape[0], None, None, C.c_void_p(d_cha.data_ptr()), None))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("workloads", nargs="*", default=["dvbs2", "c2"])
    a = ap.parse_args()
    if L.device_count() < 1:
        sys.exit("llr_io_probe needs an MI355X: no HIP device visible")
    ok = all([run(wl, a.rounds, a.warmup, a.frames) for wl in a.workloads])
    sys.exit(0 if ok else 1)
