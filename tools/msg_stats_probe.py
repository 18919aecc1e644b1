#!/usr/bin/env python3
"""What the message-label histograms cost (lut_ldpc_amd/csrc/hip/kernels_stats.hpp), one JSON line per measurement:

  launch    one histogram launch against one check-pass launch of the same counted decode (HIP events by kind, Decoder.profile()),
            DVB-S2 N=64800 (6 iterations) and N=500 (8 iterations), 8192 sampled frames, level 3, every frame at every dump
  decode    wall clock of Decoder.message_histogram against lut_decode_batch_trace + counting in numpy on the same labels:
            N=500, 8 iterations, 4096 frames, level 3, exit tests off, best of three
  trace     the trace + numpy side alone; runs on a build without the histograms too: LUTLDPC_LIB=<other build>/liblut_ldpc_amd.so

Usage: tools/msg_stats_probe.py [launch] [decode] [trace]"""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np

import lut_ldpc_amd as L

CODES = ROOT / "data" / "codes"
CASES = {"dvbs2_q4_i6": ("rate0.50_irreg_dvbs2_N64800", 6, dict(allow_degree_one=True), 32400),
         "n500_q4_i8": ("rate0.50_dv02-17_dc08-09_lut_q4_N500", 8, {}, 0)}


def lib_name():
    p = Path(L._capi.LIB_PATH).resolve()
    return str(p.relative_to(ROOT)) if ROOT in p.parents else p.name


def codec(name):
    alist, I, extra, rank = CASES[name]
    cd = L.Codec(CODES / f"{alist}.alist", known_rank=rank, device=0)
    cd.design_luts(sigma2=0.88 ** 2, max_iters=I, nq_cha=16, nq_msg=16, **extra)
    return cd, I


def launch(name, B=8192):
    cd, I = codec(name)
    dec = cd.decoder()
    cd.message_histogram(1.5, 1, 0, 0, B, level=3, mode="all")                    # buffers, tables, code objects
    dec.set_profiling(True); dec.reset_profile()
    cd.message_histogram(1.5, 1, 0, 0, B, level=3, mode="all")
    prof = dec.profile(); dec.set_profiling(False)
    h, c = prof["histogram"], prof["cn_pass"]
    hm, cm = h["ms"] / h["launches"], c["ms"] / c["launches"]
    print(json.dumps({"probe": "launch", "config": name, "B": B, "edges": cd.nedges, "histogram_launches": h["launches"], "histogram_ms_per_launch": round(hm, 4),
                      "cn_pass_launches": c["launches"], "cn_pass_ms_per_launch": round(cm, 4), "histogram_over_cn_pass": round(hm / cm, 3),
                      "kernel_ms": {k: round(v["ms"], 3) for k, v in prof.items() if v["launches"]}, "lib": lib_name()}), flush=True)
    cd.close()


def best_of(fn, n=3):
    fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter(); out = fn(); ts.append(time.perf_counter() - t0)
    return min(ts), out


def count_trace(dec, cha, msg, E, nq):
    _, _, tr = dec.lut_decode_batch_trace(cha, msg, 3, E)
    return np.stack([np.bincount(tr[k].ravel(), minlength=nq) for k in range(tr.shape[0])]).astype(np.int64)


def decode(with_histogram, B=4096):
    cd, I = codec("n500_q4_i8")
    dec = cd.decoder()
    cd.set_exit_conditions(I, False, False)
    cha, msg, _ = cd.sample_labels(1.5, 1, 0, 0, B)
    t_trace, want = best_of(lambda: count_trace(dec, cha, msg, cd.nedges, 16))
    out = {"probe": "decode" if with_histogram else "trace", "config": "n500_q4_i8", "B": B, "level": 3, "trace_plus_numpy_s": round(t_trace, 4), "lib": lib_name()}
    if with_histogram:
        t_hist, got = best_of(lambda: dec.message_histogram(cha, msg, level=3, mode="all")[0])
        assert (got[:, 0, 0, :] == want).all() and got[:, :, 1].sum() == 0
        out.update({"histogram_s": round(t_hist, 4), "trace_over_histogram": round(t_trace / t_hist, 1)})
    print(json.dumps(out), flush=True)
    cd.close()


if __name__ == "__main__":
    what = sys.argv[1:] or ["launch", "decode"]
    if "launch" in what:
        for name in CASES:
            launch(name)
    if "decode" in what:
        decode(True)
    if "trace" in what:
        decode(False)
