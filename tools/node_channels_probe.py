#!/usr/bin/env python3
"""What the per-node channel classes cost in the sampler: sample_labels_kernel with the handle's classes against the same kernel with
the caller's one table, on ONE handle of the DVB-S2 code, 16384 frames per call, in one process, the variants alternating:
  single       the caller's one table (cells != NULL): one slot in LDS, no class bytes read -- the baseline of this run
  classes 1    node channels with one class: the same table on every node, found through the class byte of each node
  classes 4    four classes in contiguous blocks of nodes (offsets 0, -inf, +inf, -3 dB): a workgroup loads one or two tables
  classes 16   16 classes v % 16 (offsets -7.5 .. 0 dB in steps of 0.5): every workgroup loads all 16 tables, every wave changes
               its table from node to node -- the worst case
Time = LUTLDPC_K_FRONTEND of the library's profile (device events around the sampler launch) of lutldpc_decoder_sample_labels;
the host copies of that entry are outside it.  2 warm-up rounds, then --rounds timed ones; median, min, max and the ratio of the
medians to `single`.  classes 1 must return the labels of single, bit for bit.
Then ber_sim end to end (lutldpc_ber_sim_run, wall time of load + one SNR point of --ber-frames frames at 1.0 dB, all-zero codeword,
LUTLDPC_PLACE=0 as the ber_sim command line sets it for runs this short; the variants take turns in going first) on the same code: without the Channel keys, with four classes that all have offset 0 (the same frames, the same counters: what the class
front end itself costs a sweep), and with the last 5 % of the nodes punctured (another channel: more frames fail, more iterations).
One JSON line at the end.
Usage: tools/node_channels_probe.py [--rounds 7] [--warmup 2] [--frames 16384] [--ber-frames 65536] [--no-ber]"""
import argparse
import ctypes as C
import json
import os
import shutil
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np

import bench
import lut_ldpc_amd as L
from lut_ldpc_amd._capi import lib

INF = float("inf")


def sampler(rounds, warmup, B):
    alist, sigma, max_iter, qc, qm, _, extra, known_rank = bench.WORKLOADS["dvbs2"]
    cd = L.Codec(ROOT / "data" / "codes" / f"{alist}.alist", known_rank=known_rank, device=0)
    cd.design_luts(sigma2=sigma * sigma, max_iters=max_iter, nq_cha=1 << qc, nq_msg=1 << qm, **extra)
    dec = cd.decoder()
    N, snr = cd.nvar, 1.0
    v = np.arange(N)
    layouts = {
        "classes 1": (np.zeros(N, np.uint8), [0.0]),
        "classes 4": ((v * 4 // N).astype(np.uint8), [0.0, -INF, INF, -3.0]),
        "classes 16": ((v % 16).astype(np.uint8), [-0.5 * k for k in range(16)]),
    }
    tables = {}
    for name, (ids, off) in layouts.items():
        cd.set_node_channels(ids, off)
        tables[name] = [cd.node_channel_cells(snr, k) for k in range(len(off))]
    cd.set_node_channels(None)
    one = cd.channel_cells(snr)
    cha, msg = np.empty((B, N), np.uint8), np.empty((B, N), np.uint8)
    keep = {}
    dec.set_profiling(True)
    ms = {k: [] for k in ["single"] + list(layouts)}
    for r in range(warmup + rounds):
        for k in ms:
            if k == "single":
                dec.set_node_channels(None)
            else:
                dec.set_node_channels(layouts[k][0], tables[k])
            dec.reset_profile()
            dec.sample_labels(one if k == "single" else None, 7, 3, 2 ** 32 - 100, B, cha=cha, msg=msg)
            p = dec.profile()["frontend"]
            assert p["launches"] == 1, p
            if r >= warmup:
                ms[k].append(p["ms"])
            if r == 0 and k in ("single", "classes 1"):
                keep[k] = (cha[:64].copy(), msg[:64].copy(), int(cha.sum(dtype=np.int64)), int(msg.sum(dtype=np.int64)))
    dec.set_profiling(False)
    dec.set_node_channels(None)
    same = all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(keep["single"], keep["classes 1"]))
    out = {"frames": B, "nvar": N, "snr_db": snr, "rounds": rounds, "warmup": warmup, "classes_1_equals_single": bool(same)}
    base = float(np.median(ms["single"]))
    print(f"sampler, DVB-S2 N = {N}, {B} frames per call, kernel time (LUTLDPC_K_FRONTEND) in ms; classes 1 equals single: {same}")
    print(f"  {'variant':12s} {'median':>9s} {'min':>9s} {'max':>9s} {'over single':>12s}")
    for k, t in ms.items():
        med = float(np.median(t))
        out[k.replace(" ", "_")] = {"ms_median": round(med, 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4), "over_single": round(med / base, 4)}
        print(f"  {k:12s} {med:9.4f} {min(t):9.4f} {max(t):9.4f} {med / base:12.4f}")
    cd.close()
    return out, same


INI = """[Sim]
   SNRdB    = 1.0
   Nframes  = {frames}
   Nfers    = 1000000000
   ber_min  = 0
   fer_min  = 0
   save_codec = -1
   batch_frames = 32768
[LDPC]
   parity_filename = rate0.50_irreg_dvbs2_N64800
   zero_codeword   = true
   known_rank = 32400
[LUT]
   max_iter = 50
   design_thr = 0.88
   qbits_channel = 4
   qbits_message_uniform = 4
   allow_degree_one = true
{channel}"""


def ber_sim(frames, rounds):
    N = 64800
    v = np.arange(N)
    variants = {
        "no keys": None,
        "4 classes, offset 0": ((v * 4 // N).astype(np.uint8), "0 0 0 0"),
        "5 % punctured": (np.where(v >= N - N // 20, 1, 0).astype(np.uint8), "0 -inf"),
    }
    out = {"frames": frames}
    with tempfile.TemporaryDirectory(prefix="node_channels_probe_") as tmp:
        base = Path(tmp)
        (base / "codes").mkdir()
        shutil.copy(ROOT / "data" / "codes" / "rate0.50_irreg_dvbs2_N64800.alist", base / "codes")
        params = {}
        for i, (name, spec) in enumerate(variants.items()):
            ch = ""
            if spec is not None:
                (base / "codes" / f"classes{i}.txt").write_text(" ".join(str(int(c)) for c in spec[0]) + "\n")
                ch = f"[Channel]\n   node_classes_filename = classes{i}.txt\n   class_snr_offset_dB = {spec[1]}\n"
            params[name] = base / f"probe{i}.ini"
            params[name].write_text(INI.format(frames=frames, channel=ch))
        secs, counters = {k: [] for k in variants}, {}
        os.environ.setdefault("LUTLDPC_PLACE", "0")
        names = list(params)
        for r in range(1 + rounds):                                    # (the first round warms code objects and the design cache)
            for name in names[r % 3:] + names[:r % 3]:
                p = params[name]
                snr, cnt = (C.c_double * 4)(), (C.c_int64 * 20)()
                t0 = time.perf_counter()
                n = lib.lutldpc_ber_sim_run(str(p).encode(), str(base).encode(), 0, f"_r{r}".encode(), 0, 0, 1, snr, cnt, 4)
                dt = time.perf_counter() - t0
                assert n == 1, L._capi.last_error()
                counters[name] = list(cnt[:5])
                if r:
                    secs[name].append(dt)
    same = counters["no keys"] == counters["4 classes, offset 0"]
    print(f"ber_sim end to end (load + {frames} frames at 1.0 dB), {rounds} rounds, wall seconds; counters of `4 classes, offset 0` equal `no keys`: {same}")
    print(f"  {'variant':22s} {'median':>8s} {'min':>8s} {'max':>8s} {'over no keys':>13s}   counters")
    base_s = float(np.median(secs["no keys"]))
    for name, t in secs.items():
        med = float(np.median(t))
        out[name] = {"s_median": round(med, 3), "s_min": round(min(t), 3), "s_max": round(max(t), 3), "over_no_keys": round(med / base_s, 4), "counters": counters[name]}
        print(f"  {name:22s} {med:8.3f} {min(t):8.3f} {max(t):8.3f} {med / base_s:13.4f}   {counters[name]}")
    out["offset_0_counters_equal"] = bool(same)
    return out, same


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=16384)
    ap.add_argument("--ber-frames", type=int, default=65536)
    ap.add_argument("--ber-rounds", type=int, default=9)
    ap.add_argument("--no-ber", action="store_true")
    a = ap.parse_args()
    if L.device_count() < 1:
        sys.exit("node_channels_probe needs an MI355X: no HIP device visible")
    res, ok = sampler(a.rounds, a.warmup, a.frames)
    out = {"sampler": res}
    if not a.no_ber:
        out["ber_sim"], ok2 = ber_sim(a.ber_frames, a.ber_rounds)
        ok = ok and ok2
    print(json.dumps(out), flush=True)
    sys.exit(0 if ok else 1)
