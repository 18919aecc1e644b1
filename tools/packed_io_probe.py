#!/usr/bin/env python3
"""What the host link costs a decode of labels the caller holds, and what lutldpc_decoder_decode_batch_packed saves of it.
Per workload (bench.py's: DVB-S2 at 32768 frames, the (3,6) N = 10000 code at 4096), in ONE process, as-shipped exit conditions
(psc and pisc), 0.4 dB above the design point, initial messages = cha2msg_map of the channel labels (QCHA):
  bytes    lutldpc_decoder_decode_batch: a byte per channel label, a byte per initial-message label in, a byte per decided bit out
  packed   lutldpc_decoder_decode_batch_packed: nibble-packed channel labels in, the map applied on the device, the data bits
           (the first nvar - rank(H)) out, one bit each
  device   lutldpc_decoder_decode_batch_device on buffers that already live in HBM: no transfer at all, the ceiling
Wall time per batch from a host clock around calls that end in a stream synchronise; all buffers exist and are touched before the
first call; 2 warm-up rounds, then 5 timed rounds with the three entries alternating; median, min and max.  The packed result is
compared with the byte entry's on every frame (data bits and iteration codes).  One JSON line per workload after the table.
Usage: tools/packed_io_probe.py [--rounds 5] [--warmup 2] [workload ...]      (default: dvbs2 c2)"""
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
from lut_ldpc_amd._capi import IN_NIBBLES, PackedIO, check, lib

u8p, i32p, u32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)


def run(wl, rounds, warmup):
    import torch
    alist, sigma, max_iter, qc, qm, B, extra, known_rank = bench.WORKLOADS[wl]
    cd = L.Codec(ROOT / "data" / "codes" / f"{alist}.alist", known_rank=known_rank, device=0)
    cd.design_luts(sigma2=sigma * sigma, max_iters=max_iter, nq_cha=1 << qc, nq_msg=1 << qm, **extra)
    cd.set_initial_message_mode(1)
    cd.set_exit_conditions(max_iter, True, True)
    N, K = cd.nvar, cd.ninfo
    snr = -10 * np.log10(2 * cd.rate * sigma * sigma) + 0.4
    mp = np.ascontiguousarray(cd.cha2msg_map, np.int32)
    # labels made in HBM (bench.py), one copy kept there for the device entry, one brought to the host in both formats
    d_cha, d_msg = bench.make_labels_device(cd, B, snr, seed=56, qcha_map=mp)
    cha, msg = d_cha.cpu().numpy(), d_msg.cpu().numpy()
    nib = (d_cha[:, 0::2] | (d_cha[:, 1::2] << 4)).contiguous().cpu().numpy()
    assert N % 2 == 0 and nib.shape == (B, N // 2) and (nib[:64] == packing.pack_nibbles(cha[:64])).all()
    d_bits = torch.zeros((B, N), dtype=torch.uint8, device="cuda")
    d_its = torch.zeros(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    W = (K + 31) // 32
    bits, its = np.zeros((B, N), np.uint8), np.zeros(B, np.int32)          # (zeros, not empty: the pages exist before the first copy)
    words, its_p = np.zeros((B, W), np.uint32), np.zeros(B, np.int32)
    h = C.c_void_p(lib.lutldpc_codec_decoder(cd._h))
    io = PackedIO(IN_NIBBLES, mp.ctypes.data_as(i32p), 0, K)
    entries = {
        "bytes": lambda: check(lib.lutldpc_decoder_decode_batch(h, cha.ctypes.data_as(u8p), msg.ctypes.data_as(u8p), B, bits.ctypes.data_as(u8p), its.ctypes.data_as(i32p))),
        "packed": lambda: check(lib.lutldpc_decoder_decode_batch_packed(h, C.byref(io), nib.ctypes.data_as(u8p), None, B, words.ctypes.data_as(u32p), its_p.ctypes.data_as(i32p))),
        "device": lambda: check(lib.lutldpc_decoder_decode_batch_device(h, C.c_void_p(d_cha.data_ptr()), C.c_void_p(d_msg.data_ptr()), B, C.c_void_p(d_bits.data_ptr()),
                                                                         C.c_void_p(d_its.data_ptr()), 1)),
    }
    moved = {"bytes": (2 * B * N, B * N + 4 * B), "packed": (B * (N // 2), 4 * B * W + 4 * B), "device": (0, 0)}
    ms = {k: [] for k in entries}
    for r in range(warmup + rounds):
        for k, call in entries.items():
            t0 = time.perf_counter()
            call()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= warmup:
                ms[k].append(dt)
    same = bool((its == its_p).all() and (packing.unpack_bits(words, K) == bits[:, :K]).all() and (d_its.cpu().numpy() == its).all())
    out = {"workload": wl, "B": B, "nvar": N, "K_info": K, "snr_db": round(float(snr), 3), "rounds": rounds, "warmup": warmup, "packed_equals_bytes": same,
           "converged": int((its > 0).sum() + (its == 0).sum()), "failed": int((its < 0).sum())}
    print(f"{wl}: {B} frames, N = {N}, K = {K}, {snr:.2f} dB, {out['converged']} frames converged, {out['failed']} failed; packed result equals the byte entry's: {same}")
    print(f"  {'entry':8s} {'MB in':>9s} {'MB out':>9s} {'median ms':>10s} {'min ms':>9s} {'max ms':>9s} {'frames/s':>10s}")
    for k in entries:
        med = float(np.median(ms[k]))
        out[k] = {"bytes_in": moved[k][0], "bytes_out": moved[k][1], "ms_median": round(med, 2), "ms_min": round(min(ms[k]), 2), "ms_max": round(max(ms[k]), 2)}
        print(f"  {k:8s} {moved[k][0] / 1e6:9.1f} {moved[k][1] / 1e6:9.1f} {med:10.2f} {min(ms[k]):9.2f} {max(ms[k]):9.2f} {B / med * 1e3:10.0f}")
    out["packed_over_bytes_time"] = round(out["packed"]["ms_median"] / out["bytes"]["ms_median"], 3)
    out["packed_over_device_time"] = round(out["packed"]["ms_median"] / out["device"]["ms_median"], 2)
    print(json.dumps(out), flush=True)
    cd.close()
    return same


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("workloads", nargs="*", default=["dvbs2", "c2"])
    a = ap.parse_args()
    if L.device_count() < 1:
        sys.exit("packed_io_probe needs an MI355X: no HIP device visible")
    ok = all([run(wl, a.rounds, a.warmup) for wl in a.workloads])
    sys.exit(0 if ok else 1)
