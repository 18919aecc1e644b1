#!/usr/bin/env python3
"""bench.py -- decoded codewords/s of the MI355X LUT-LDPC decode path.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload dvbs2|twin|c2|c1|c5|c5chk] [--batch B] [--mode fixed|shipped]
                    [--dump-outputs DIR] [--full [--no-configs] [--no-cpu-baseline] ...]

A *step* is one pass of the hot path (LDPC_Code_LUT::lut_decode, all iterations) over one batch of
B frames per GPU whose quantised labels are already resident in HBM.  Default workload: the
configuration BASELINE.json's metric is quoted on -- rate0.50_irreg_dvbs2_N64800, 4-bit channel and
message labels, 50 iterations, min-LUT -- in fixed-work mode (parity_check_iter = false: every frame
runs all 50 iterations, nothing is skipped).  For N > 1 launch through torch.distributed.run: one
process per GPU, frames sharded (weak scaling), one RCCL all-reduce of the BER/FER counters.

Prints ONE JSON line (rank 0).  `value` and `ms_per_step` come from K timed steps in the production configuration (from
its second call on, a decode of a given batch size is replayed as one hipGraph launch).  A plain run does nothing else:
set-up, W warm-up steps, the K timed steps, the outputs of the last step when --dump-outputs DIR is given, the line.

--dump-outputs DIR: what the last timed step computed, as float32 / float64 .npy files (rank 0's frames; the inputs are
seeded, so runs with the same arguments decode the same frames): iterations.npy (iteration count of every frame, negative =
not converged), ones_per_frame.npy (set decided bits of every frame: bit errors, the codeword is all-zero), bits.npy with
bits_frames.npy (the decided bits of a fixed, seeded sample of the frames, at most 32 MB, and their frame indices),
counters.npy (frames, data bits, frame errors, data bit errors, uncoded bit errors, summed over ranks).

--full adds everything measured beside the headline figure, each after the timed region and never part of `value`:
`single_steps` (--reps steps timed one by one, with socket power and shader clock).  `roofline` is for the dominant kernel --
pass_fused_kernel, which runs the check pass of one half of the frame groups together with the variable pass of the other
half (2 x iterations launches per decode) --: algorithmic bytes per launch / mean launch duration from HIP events recorded
on the decoder's own stream while the same K steps are issued once more as plain launches right after the timed region
(events cannot be recorded inside a graph replay).  `frame_loop` adds the device channel sampler and
the error counting around the decode (the whole loop of LDPC_BER_Sim::sim_snr_point); `as_shipped` is the
same decoder with the reference's default exit test on (parity_check_iter = true), a few extra steps.
`cpu_baseline` times the oracle (oracle/, the CPU restatement of the reference decoder) on a bounded
sample of the same workload on this host -- the oracle is used only there.  `configs` (one GPU) times the other
BASELINE.json configurations as well -- (3,6) N=10000 at batch 4096, (6,32) N=2048 with both check updates, the N=64800 twin,
the N=500 example code -- each with its throughput in both exit modes, the dominant kernel with its mean launch time from HIP
events, the roofline fraction recomputed from SURVEY 8(d)'s bytes, and an oracle check of a sample.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))
# LUT designs are kept between runs (lut_ldpc_amd/csrc/host/ldpc_code_lut.cpp, "design cache"): set-up, never timed
os.environ.setdefault("LUTLDPC_DESIGN_CACHE", str(ROOT / "data" / "design_cache"))
try:
    Path(os.environ["LUTLDPC_DESIGN_CACHE"]).mkdir(parents=True, exist_ok=True)
except OSError:
    pass

HBM_PEAK_GBPS = 8000.0      # MI355X HBM3E spec

WORKLOADS = {
    # name: (alist, design sigma, max_iter, qbits_cha, qbits_msg, default batch, extra design kwargs, known rank)
    # 32768 frames per step (6.8 GB of rows): +7 % over 4096 (shorter launch tails relative to the launch), and 0-2 % (fixed
    # work) / +3 % (as shipped: halves of 32 frame groups, the most the compaction takes, retire at a finer grain) over 16384
    "dvbs2": ("rate0.50_irreg_dvbs2_N64800", 0.88, 50, 4, 4, 32768, dict(allow_degree_one=True), 32400),
    "twin": ("rate0.50_dv02-08_dc07-08_lut_q4_N64800", 0.88, 50, 4, 4, 32768, {}, 32400),
    "c2": ("rate0.50_dv03_dc06_N10000", 0.84, 50, 4, 4, 4096, {}, 5000),
    "c1": ("rate0.50_dv02-17_dc08-09_lut_q4_N500", 0.88, 50, 4, 4, 16384, {}, 250),
    # params/ber.ini.regular.example: (6,32) N=2048, rank 325, 3-bit messages, 8 iterations, trees from a file, QCHA
    # initial messages, design at Eb/N0 = 3.9 dB (sigma^2 = 1 / (2 R 10^0.39)); c5chk: CHKTREE check update (min_lut = false)
    # (36864 frames = 4608 sets of 8 = six full rounds of the 768 workgroups the chip holds at once (three 51 KB workgroups per
    # compute unit): 32768 frames end on a sixth round that is one third full, -11 %)
    "c5": ("rate0.84_reg_v6c32_N2048", 0.6159, 8, 4, 3, 36864, dict(tree_method="filename=" + str(ROOT / "data" / "trees" / "6_32_wide.ini")), 325),
    "c5chk": ("rate0.84_reg_v6c32_N2048", 0.6159, 8, 4, 3, 32768,
              dict(tree_method="filename=" + str(ROOT / "data" / "trees" / "6_32_wide.ini"), min_lut=False), 325),
}


def make_labels(cd, B, snr_db, seed, qcha_map=None):
    """All-zero codeword over BPSK/AWGN (src/LDPC_BER_Sim.cpp:248-278) quantised with the designed
    boundaries; generated on the host once, outside the timed region."""
    rng = np.random.default_rng(seed)
    N0 = 10 ** (-snr_db / 10) / cd.rate
    qc, qm = cd.qb_cha, cd.qb_msg
    cha = np.empty((B, cd.nvar), np.uint8)
    msg = np.empty((B, cd.nvar), np.uint8)
    step = max(1, (1 << 24) // cd.nvar)
    for b0 in range(0, B, step):
        x = 1.0 + rng.normal(0.0, np.sqrt(N0 / 2), (min(step, B - b0), cd.nvar))
        llr = 4 * x / N0
        # quant_nonlin: number of boundaries strictly below the value (src/common.cpp:120-129)
        cha[b0:b0 + len(llr)] = np.searchsorted(qc, llr, side="left").astype(np.uint8)
        if qcha_map is None:
            msg[b0:b0 + len(llr)] = np.searchsorted(qm, llr, side="left").astype(np.uint8)
        else:                       # QCHA: initial message = Nq_Cha_2_Nq_Msg_map[channel label] (src/LDPC_Code_LUT.cpp:216-220)
            msg[b0:b0 + len(llr)] = qcha_map[cha[b0:b0 + len(llr)]]
    return cha, msg


def make_labels_device(cd, B, snr_db, seed, qcha_map=None):
    """The same synthetic frames generated in HBM (torch's Philox normal generator + bucketize = quant_nonlin): a 16384-frame
    DVB-S2 batch is 10^9 samples, which numpy needs ~20 s for.  Untimed set-up either way; the CPU baseline decodes a copy of
    the first frames of exactly these labels."""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    N0 = 10 ** (-snr_db / 10) / cd.rate
    qc = torch.from_numpy(np.ascontiguousarray(cd.qb_cha)).cuda()
    qm = torch.from_numpy(np.ascontiguousarray(cd.qb_msg)).cuda()
    qmap = None if qcha_map is None else torch.from_numpy(np.ascontiguousarray(qcha_map, np.uint8)).cuda()
    cha = torch.empty((B, cd.nvar), dtype=torch.uint8, device="cuda")
    msg = torch.empty((B, cd.nvar), dtype=torch.uint8, device="cuda")
    step = max(1, (1 << 27) // cd.nvar)
    for b0 in range(0, B, step):
        n = min(step, B - b0)
        llr = (1.0 + torch.randn((n, cd.nvar), generator=g, device="cuda", dtype=torch.float64) * float(np.sqrt(N0 / 2))) * (4.0 / N0)
        c = torch.bucketize(llr, qc, right=False)            # number of boundaries strictly below the value (src/common.cpp:120-129)
        cha[b0:b0 + n] = c.to(torch.uint8)
        msg[b0:b0 + n] = torch.bucketize(llr, qm, right=False).to(torch.uint8) if qmap is None else qmap[c]
    # The decoder runs on its OWN (non-blocking) HIP stream: the labels must be complete, and torch must be done with the temporaries
    # it has already handed back to its caching allocator, before anything on that stream touches memory torch may reuse -- a
    # decode started here without this wait reads half-written labels, and its output buffer (a fresh torch.empty) can land on the
    # freed `llr` block while torch's kernels still read it.
    del llr, c
    torch.cuda.synchronize()
    return cha, msg


class PowerSampler:
    """Socket power and shader clock from the amdgpu hwmon files, sampled by a thread while the GPU works (a few ms per
    sample, no GPU access).  Identical runs land on discrete throughput levels per process; the
    samples say whether a level comes with a different clock or power.  Silent when the files are not there."""

    def __init__(self, period_s=0.01, pci=None):
        import glob
        self.period = period_s
        # the hwmon directory of THIS GPU (a box shows the cards of the whole host): by PCI address when known
        roots = []
        if pci:
            roots = sorted(glob.glob(f"/sys/bus/pci/devices/{pci}/hwmon/hwmon*"))
        if not roots:
            roots = sorted(glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*"))
        self.card = roots[0] if roots else None
        self.matched_by_pci = bool(pci and roots and pci in roots[0]) or bool(pci and roots and "/sys/bus/pci/devices/" in roots[0])
        pick = lambda names: [f"{self.card}/{n}" for n in names if self.card and os.path.exists(f"{self.card}/{n}")][:1]
        self.power = pick(["power1_average", "power1_input"])
        self.sclk = pick(["freq1_input"])
        self.samples = []
        self._stop = False
        self._thr = None

    def _read(self, paths):
        try:
            return float(open(paths[0]).read().split()[0]) if paths else None
        except (OSError, ValueError, IndexError):
            return None

    def __enter__(self):
        import threading

        def loop():
            while not self._stop:
                self.samples.append((time.perf_counter(), self._read(self.power), self._read(self.sclk)))
                time.sleep(self.period)
        if self.power or self.sclk:
            self._thr = threading.Thread(target=loop, daemon=True)
            self._thr.start()
        return self

    def __exit__(self, *a):
        self._stop = True
        if self._thr:
            self._thr.join()

    def summary(self):
        pw = [p * 1e-6 for _, p, _ in self.samples if p is not None]
        ck = [c * 1e-6 for _, _, c in self.samples if c is not None]
        if not pw and not ck:
            return None
        q = lambda v, f: float(np.percentile(v, f)) if v else None
        return {"samples": len(self.samples), "hwmon": self.card, "matched_by_pci_address": self.matched_by_pci, "socket_power_W": {"median": q(pw, 50), "p10": q(pw, 10), "p90": q(pw, 90)},
                "sclk_MHz": {"median": q(ck, 50), "p10": q(ck, 10), "p90": q(ck, 90)}}


def usable_cores() -> int:
    """Cores this process may really use: the scheduler affinity, capped by the cgroup CPU quota (a GPU box hands a job a
    share of the host's cores, which os.cpu_count() does not show)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(int(txt[0]) / int(txt[1]))))
            else:
                q = int(txt[0])
                if q > 0:
                    n = min(n, max(1, q // int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())))
        except (OSError, ValueError, IndexError):
            pass
    return max(1, n)


def oracle_codec_for(cd, max_iter, psc, pisc):
    """The oracle (oracle/: CPU restatement of the reference decoder) loaded with the product's tables, handed over as the
    reference's own tree text.  Checker only: called after the timed regions."""
    from oracle import oracle as orc
    code = orc.Code(ROOT / "data" / "codes" / f"{cd.alist}.alist")
    oc = orc.Codec(code, skip_rank=True)
    nq = np.full(max_iter, cd.nq_msg, np.int32)
    oc.set_trees_txt(cd.var_trees_txt, "" if cd.min_lut else cd.chk_trees_txt, max_iter, np.zeros(max_iter, np.uint8), cd.nq_cha, nq, cd.min_lut)
    oc.set_exit_conditions(max_iter, psc, pisc)
    return oc


def outcome_sample(it, n, I):
    """n frames covering every kind of outcome of an as-shipped decode: failed, passed on the channel decisions, early exits over
    the range of iteration counts, full count -- drawn from the whole batch (both halves, every frame group)."""
    rng = np.random.default_rng(5)
    pos = it[(it > 0) & (it < I)]
    cuts = np.unique(np.percentile(pos, [0, 25, 50, 75, 100])) if len(pos) else np.array([1, I])
    groups = [np.flatnonzero(it < 0), np.flatnonzero(it == 0), np.flatnonzero(it == I)]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        groups.append(np.flatnonzero((it >= lo) & (it <= hi) & (it > 0) & (it < I)))
    idx = []
    for g in groups:
        if len(g):
            idx += list(rng.choice(g, size=min(len(g), max(1, n // len(groups))), replace=False))
    idx = list(dict.fromkeys(int(i) for i in idx))[:n]
    rest = np.setdiff1d(np.arange(len(it)), idx)
    if len(idx) < n and len(rest):
        idx += list(rng.choice(rest, size=min(len(rest), n - len(idx)), replace=False))
    return np.array(sorted(idx))


def cpu_baseline(cd, cha, msg, max_iter, psc, budget_s=9.0):
    """SURVEY 8(d), both CPU legs, on bounded samples of the same labels on this host's cores:
    (i) the oracle in FAITHFUL mode -- the reference's structure (per-output queue copy + recursive tree walk, one
        thread: ber_sim is single-threaded);
    (ii) the oracle in FLAT-TABLE mode (oracle/or_flat.c: trees flattened to arrays, one frame per thread, all cores).
    Tables are handed over as the reference's tree text.  Returns the JSON object and the decoded sample of leg (i)."""
    from oracle import oracle as orc
    code = orc.Code(ROOT / "data" / "codes" / f"{cd.alist}.alist")
    oc = orc.Codec(code, skip_rank=True)
    nq = np.full(max_iter, cd.nq_msg, np.int32)
    oc.set_trees_txt(cd.var_trees_txt, "" if cd.min_lut else cd.chk_trees_txt, max_iter, np.zeros(max_iter, np.uint8), cd.nq_cha, nq, cd.min_lut)
    oc.set_exit_conditions(max_iter, psc, psc)
    t0 = time.perf_counter()
    oc.lut_decode_batch(cha[:1], msg[:1])
    t1 = time.perf_counter() - t0
    n = int(max(2, min(len(cha), budget_s / max(t1, 1e-6))))
    t0 = time.perf_counter()
    bits, iters = oc.lut_decode_batch(cha[:n], msg[:n])
    dt = time.perf_counter() - t0
    faithful = {"value": n / dt, "unit": "codewords/s", "cores": 1,
                "sample": f"{n} frames, oracle faithful mode (per-output queue copy + recursive tree walk), {dt:.1f} s"}
    cores = usable_cores()
    t0 = time.perf_counter()
    oc.lut_decode_batch_flat(cha[:cores], msg[:cores], threads=cores)
    t1 = (time.perf_counter() - t0) / 1.0
    nf = int(max(cores, min(len(cha), cores * budget_s / max(t1, 1e-6))))
    t0 = time.perf_counter()
    fb, fi = oc.lut_decode_batch_flat(cha[:nf], msg[:nf], threads=cores)
    dtf = time.perf_counter() - t0
    m = min(n, nf)
    flat = {"value": nf / dtf, "unit": "codewords/s", "cores": cores,
            "sample": f"{nf} frames, oracle flat-table mode (trees flattened to arrays, one frame per thread), {dtf:.1f} s",
            "matches_faithful_mode": bool((fb[:m] == bits[:m]).all() and (fi[:m] == iters[:m]).all())}
    return {"value": flat["value"], "unit": "codewords/s", "cores": cores, "kind": "port",
            "sample": flat["sample"] + f"; nproc = {cores}", "faithful_1core": faithful, "flat_allcores": flat}, bits, iters, fb, fi


def algorithmic_bytes_per_frame(E, N, I, b):
    """bytes = 4 I E b + (I + 2) N b + N / 8 (b bytes per stored label; I executed iterations)"""
    return (4 * I * E + (I + 2) * N) * b + N / 8


KERNEL_OF_KIND = {"resident": "lutldpc_jit_pass (generated LDS-resident decode: all iterations in one launch)",
                  "fused_pass": "pass_fused_kernel (check pass of one half-batch + variable pass of the other)",
                  "cn_pass": "check pass", "vn_pass": "variable pass", "decision": "decision pass", "syndrome": "syndrome_bits_kernel",
                  "layout": "transposes / state", "frontend": "sampler + error count"}


def quick_config(L, torch, wl, B, device, steps=4, oracle_frames=32):
    """One of the other BASELINE configurations: throughput on HBM-resident labels in both exit modes, the dominant kernel with its
    mean launch duration (HIP events on the decoder's stream, plain launches after the timed region), the roofline fraction of
    the whole decode from SURVEY 8(d)'s bytes, and an oracle check of a sample of each mode's output."""
    alist, sigma, max_iter, qc, qm, B_default, extra, known_rank = WORKLOADS[wl]
    B = B or B_default
    t_all = time.perf_counter()
    cd = L.Codec(ROOT / "data" / "codes" / f"{alist}.alist", known_rank=known_rank, device=device)
    cd.alist, cd.nq_cha, cd.nq_msg = alist, 1 << qc, 1 << qm
    cd.design_luts(sigma2=sigma * sigma, max_iters=max_iter, nq_cha=1 << qc, nq_msg=1 << qm, **extra)
    cd.min_lut = bool(extra.get("min_lut", True))
    qmap = None
    if wl.startswith("c5"):
        cd.set_initial_message_mode(1)
        qmap = np.asarray(cd.cha2msg_map, np.uint8)
    N, E = cd.nvar, cd.nedges
    out = {"workload": f"{alist}, {qc}-bit channel / {qm}-bit messages, {max_iter} iterations, {'min-LUT' if cd.min_lut else 'CHKTREE check update'}",
           "frames_per_step": B, "N": N, "E": E}
    bits = torch.empty((B, N), dtype=torch.uint8, device="cuda")
    its = torch.empty(B, dtype=torch.int32, device="cuda")
    for mode, psc in (("fixed", False), ("as_shipped", True)):
        snr = -10 * np.log10(2 * cd.rate * sigma * sigma) + (0.4 if psc else 0.0)
        cd.set_exit_conditions(max_iter, psc, psc)
        dec = cd.decoder()
        cha, msg = make_labels_device(cd, B, snr, seed=777 + psc, qcha_map=qmap)

        def step(sync):
            dec.lut_decode_batch_device(cha.data_ptr(), msg.data_ptr(), B, bits.data_ptr(), its.data_ptr(), sync=sync)
        for _ in range(3):                                   # plain launches, graph capture, first replay
            step(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(steps):
            step(k == steps - 1)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        it_h = its.cpu().numpy()
        it_eff = float(np.abs(it_h).mean()) if psc else float(max_iter)
        b_msg = float(dec.describe()["message_bytes"])
        entry = {"value": B / dt, "unit": "codewords/s", "ms_per_step": dt * 1e3, "EbN0_dB": round(float(snr), 3), "mean_iterations_executed": it_eff}
        if not psc:
            dec.set_profiling(True); dec.reset_profile()
            step(True)
            prof = {k: v for k, v in dec.profile().items() if v["launches"]}
            dec.set_profiling(False)
            kind = max(prof, key=lambda k: prof[k]["ms"])
            name = KERNEL_OF_KIND.get(kind, kind)
            if kind in ("cn_pass", "vn_pass"):
                cls = dec.describe()["cn_classes" if kind == "cn_pass" else "vn_classes"]
                name = f"{cls[0]['kernel']} ({name})"
            bpf = algorithmic_bytes_per_frame(E, N, max_iter, b_msg)
            entry.update({"dominant_kernel": name, "dominant_kernel_avg_launch_ms": prof[kind]["ms"] / prof[kind]["launches"],
                          "dominant_kernel_launches_per_step": prof[kind]["launches"], "dominant_kernel_share_of_kernel_time": prof[kind]["ms"] / sum(v["ms"] for v in prof.values()),
                          "kernel_ms_per_step": {k: v["ms"] for k, v in prof.items()},
                          "roofline": {"bound": "hbm", "algorithmic_bytes_per_frame": bpf, "bytes_per_label": b_msg, "achieved": bpf * (B / dt) / 1e9, "peak": HBM_PEAK_GBPS,
                                       "unit": "GB/s", "frac": bpf * (B / dt) / 1e9 / HBM_PEAK_GBPS,
                                       "note": ("messages stay in LDS for the whole decode: the HBM traffic is the labels in and the bits out; the fraction is the "
                                                "canonical SURVEY 8(d) bytes over the decode time, comparable with the streaming kernels" if kind == "resident" else
                                                "SURVEY 8(d) bytes of the whole decode over its wall time")}})
        # oracle check on a sample (psc: every kind of outcome), after the timed region
        idx = outcome_sample(it_h, oracle_frames, max_iter) if psc else np.arange(min(B, oracle_frames))
        sel = torch.from_numpy(idx).cuda()
        oc = oracle_codec_for(cd, max_iter, psc, psc)
        wb, wi = oc.lut_decode_batch_flat(cha[sel].cpu().numpy(), msg[sel].cpu().numpy(), threads=usable_cores())
        entry["gpu_matches_oracle_on_sample"] = bool((wi == it_h[idx]).all() and (wb == bits[sel].cpu().numpy()).all())
        entry["frames_compared_with_oracle"] = int(len(idx))
        out[mode] = entry
        del cha, msg
    out["resident_decoder"] = bool(dec.describe().get("resident", 0))
    out["seconds"] = time.perf_counter() - t_all
    cd.close()
    del bits, its
    torch.cuda.empty_cache()
    if not (out["fixed"]["gpu_matches_oracle_on_sample"] and out["as_shipped"]["gpu_matches_oracle_on_sample"]):
        raise SystemExit(f"configs[{wl}]: GPU output differs from the oracle on the sample")
    return out


DUMP_BITS_BYTES = 32 << 20     # bits.npy: at most this many bytes of float32 decided bits (a seeded sample of the frames)


def dump_outputs(dest, out_bits, out_iters, counters):
    """What the last timed step handed its caller, as .npy files under `dest` (float32; the counters float64): the iteration
    count and the number of set decided bits of every frame, the decided bits of a fixed, seeded sample of the frames with
    their indices, and the BER/FER counters."""
    import torch
    dest.mkdir(parents=True, exist_ok=True)
    B, N = out_bits.shape
    n = min(B, max(1, DUMP_BITS_BYTES // (4 * N)))
    idx = np.arange(B) if n == B else np.sort(np.random.default_rng(0).choice(B, size=n, replace=False))
    sel = torch.from_numpy(idx).to(out_bits.device)
    np.save(dest / "bits.npy", out_bits[sel].cpu().numpy().astype(np.float32))
    np.save(dest / "bits_frames.npy", idx.astype(np.float64))
    np.save(dest / "iterations.npy", out_iters.cpu().numpy().astype(np.float32))
    np.save(dest / "ones_per_frame.npy", out_bits.sum(dim=1, dtype=torch.int32).cpu().numpy().astype(np.float32))
    np.save(dest / "counters.npy", counters.cpu().numpy().astype(np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="dvbs2", choices=sorted(WORKLOADS))
    ap.add_argument("--batch", type=int, default=0, help="frames per GPU per step")
    ap.add_argument("--mode", default="fixed", choices=["fixed", "shipped"],
                    help="fixed: parity_check_iter=false (all iterations); shipped: syndrome checks + early termination")
    ap.add_argument("--snr", type=float, default=None, help="Eb/N0 in dB of the synthetic frames")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/<name>.npy (float32 / float64, rank 0's frames)")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside the headline figure: single steps, per-kernel HIP events and rooflines, "
                         "device copy bandwidth, frame loop, as-shipped mode, the other BASELINE configurations, CPU baseline "
                         "and oracle checks (the options below apply to --full only)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--reps", type=int, default=7, help="extra single steps, each timed on its own, for the median / spread of a step (0 = skip)")
    ap.add_argument("--no-kernel-events", action="store_true", help="diagnostic: do not bracket the kernels with HIP events")
    ap.add_argument("--dist-backend", default="nccl", help="nccl (= RCCL, the real thing) or gloo (rehearsal: ranks may share a GPU)")
    ap.add_argument("--as-shipped-steps", type=int, default=3, help="extra untimed-for-`value` steps with the exit test on (0 = skip; fixed mode only)")
    ap.add_argument("--frame-loop-steps", type=int, default=2, help="extra untimed-for-`value` steps of the full sampler+decode+count loop (0 = skip)")
    ap.add_argument("--no-configs", action="store_true", help="skip the `configs` block (the other BASELINE configurations; default run on one GPU only)")
    args = ap.parse_args()

    import torch
    import lut_ldpc_amd as L

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available() or L.device_count() < 1:
        raise SystemExit("bench.py needs an MI355X (no HIP device visible); there is no CPU fallback")
    if args.dist_backend != "nccl":
        local %= torch.cuda.device_count()        # rehearsal of the N > 1 path on a box with fewer GPUs than ranks
    torch.cuda.set_device(local)
    dist = None
    # BENCH_DIST_FORCE=1: a process group for ONE rank too (under torch.distributed.run --nproc-per-node 1) -- the rehearsal of the RCCL
    # calls of the N > 1 path (init with device_id, barrier, int64 / float64 all-reduce) on a one-GPU box
    if world > 1 or os.environ.get("BENCH_DIST_FORCE"):
        import torch.distributed as dist
        if args.dist_backend == "nccl":           # RCCL over xGMI, one GPU per rank
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(args.dist_backend)

    alist, sigma, max_iter, qc, qm, B_default, extra, known_rank = WORKLOADS[args.workload]
    B = args.batch or B_default
    psc = args.mode == "shipped"

    # ---- set-up (untimed): alist -> design LUTs by density evolution -> HIP decoder --------------
    cd = L.Codec(ROOT / "data" / "codes" / f"{alist}.alist", known_rank=known_rank, device=local)
    cd.alist, cd.nq_cha, cd.nq_msg = alist, 1 << qc, 1 << qm
    cd.design_luts(sigma2=sigma * sigma, max_iters=max_iter, nq_cha=1 << qc, nq_msg=1 << qm, **extra)
    cd.set_exit_conditions(max_iter, psc, psc)
    cd.min_lut = bool(extra.get("min_lut", True))
    # fixed work: the design point itself (sigma^2 = N0/2, N0 = 10^(-snr/10)/R); as shipped: a point where frames converge
    snr = args.snr if args.snr is not None else (-10 * np.log10(2 * cd.rate * sigma * sigma) + (0.0 if not psc else 0.4))
    dec = cd.decoder()
    N, E, I = cd.nvar, cd.nedges, max_iter

    qcha_map = None
    if args.workload.startswith("c5"):
        cd.set_initial_message_mode(1)
        qcha_map = np.asarray(cd.cha2msg_map, np.uint8)
    cha, msg = make_labels_device(cd, B, snr, seed=1234 + rank, qcha_map=qcha_map)
    n_host = min(B, 4096)                                      # what the CPU baseline may sample from
    if args.full:
        cha_h, msg_h = cha[:n_host].cpu().numpy(), msg[:n_host].cpu().numpy()
    out_bits = torch.empty((B, N), dtype=torch.uint8, device="cuda")
    out_iters = torch.empty(B, dtype=torch.int32, device="cuda")
    counters = torch.zeros(5, dtype=torch.int64, device="cuda")   # frames, data bits, frame errs, bit errs, uncoded errs

    def step(sync):
        dec.lut_decode_batch_device(cha.data_ptr(), msg.data_ptr(), B, out_bits.data_ptr(), out_iters.data_ptr(), sync=sync)

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    K_info = N - cd.rank
    # slicer errors of the input labels: a property of the (fixed) synthetic input, computed once before the timed region
    uncoded = (cha < (1 << qc) // 2).sum(dtype=torch.int64)

    def count_errors():
        # BER/FER counters of the last step (src/LDPC_BER_Sim.hpp:80-85 payload), summed over ranks: ONE pass over the decided
        # data bits (all-zero codeword: a set bit is an error) gives the errors per frame, the counters follow from those
        per_frame = out_bits[:, :K_info].sum(dim=1, dtype=torch.int32)
        counters[0] = B
        counters[1] = B * K_info
        counters[2] = (per_frame > 0).sum()
        counters[3] = per_frame.sum(dtype=torch.int64)
        counters[4] = uncoded
        if dist is not None:
            dist.all_reduce(counters)

    for _ in range(max(args.warmup, 1) if args.warmup else 0):
        step(True)
    if args.warmup:
        count_errors()          # torch / RCCL lazy initialisation stays outside the timed region
    # ---- timed region: the production configuration (each decode replayed as one hipGraph launch) ----
    dec.set_profiling(False)
    barrier()
    t0 = time.perf_counter()
    for k in range(args.steps):
        step(k == args.steps - 1)
    t_decode = time.perf_counter() - t0
    count_errors()
    barrier()
    dt = time.perf_counter() - t0
    if dist is not None:
        tmax = torch.tensor([dt], dtype=torch.float64, device="cuda")
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
    frames = B * args.steps * world
    value = frames / dt
    it_exec = float(out_iters.abs().float().mean().item())
    if rank == 0 and args.dump_outputs:
        dump_outputs(Path(args.dump_outputs), out_bits, out_iters, counters)
    result = {
        "metric": "decoded codewords/sec, DVB-S2 N=64800 4-bit LUT 50-iter" if args.workload == "dvbs2" else "decoded codewords/sec",
        "value": value, "unit": "codewords/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "u8", "data": "synthetic",
        "coded_bits_per_s": value * N,
        "config": {"workload": f"{alist}, {qc}-bit channel / {qm}-bit messages, {max_iter} iterations, min-LUT, "
                               f"{'fixed work (parity_check_iter=false)' if not psc else 'as shipped (syndrome checks, early termination)'}",
                   "frames_per_gpu_per_step": B, "N": N, "E": E, "design_sigma": sigma, "EbN0_dB": round(float(snr), 3),
                   "mean_iterations_executed": it_exec, "parallelism": f"frames sharded over {world} GPU(s), counters all-reduced" + (f" ({dist.get_backend()} process group)" if dist is not None else ""),
                   "kernels": dec.describe()},
        "decode_ms_per_step_host_clock": t_decode / args.steps * 1e3,
        "counters": {"frames": int(counters[0]), "data_bits": int(counters[1]), "frame_errors": int(counters[2]),
                     "data_bit_errors": int(counters[3]), "uncoded_bit_errors": int(counters[4])},
        "full": args.full,
    }
    if args.full:
        # ---- single steps, each timed on its own (after the timed region, never part of `value`): median and spread of a step
        # inside this process, with socket power and shader clock sampled meanwhile
        step_stats = None
        if args.reps > 0:
            ts = []
            try:
                pr = torch.cuda.get_device_properties(local)
                pci = f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}.0"
            except Exception:
                pci = None
            with PowerSampler(pci=pci) as ps:
                for _ in range(args.reps):
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    step(True)
                    ts.append((time.perf_counter() - t1) * 1e3)
            step_stats = {"reps": args.reps, "median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)),
                          "codewords_per_s_at_median": B / (float(np.median(ts)) * 1e-3), "power_clock": ps.summary()}
        # ---- the same K steps again with every launch bracketed by HIP events on the decoder's stream: the
        # per-kernel durations behind `roofline` (events cannot sit inside a graph replay, so this pass issues
        # plain launches; its own wall time is reported as ms_per_step_instrumented, never as `value`)
        dec.set_profiling(not args.no_kernel_events)
        dec.reset_profile()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for k in range(args.steps if not args.no_kernel_events else 0):
            step(k == args.steps - 1)
        torch.cuda.synchronize()
        dt_instr = time.perf_counter() - t1
        prof = dec.profile()
        dec.set_profiling(False)

        vn, cn, fu = prof["vn_pass"], prof["cn_pass"], prof["fused_pass"]
        vn_ms = vn["ms"] / max(vn["launches"], 1) or float("nan")
        cn_ms = cn["ms"] / max(cn["launches"], 1) or float("nan")
        fu_ms = fu["ms"] / max(fu["launches"], 1) or float("nan")
        b_msg = float(dec.describe()["message_bytes"])      # bytes per stored label: 1 (byte rows) or 0.5 (nibble rows)
        vn_bytes = (2 * E + N) * b_msg * B                  # read E, write E, read cha (N)
        cn_bytes = 2 * E * b_msg * B
        if psc:
            vn_bytes += N * b_msg * B                       # hard-decision rows written for the syndrome test
        it_eff = it_exec if psc else float(I)
        # measured device copy bandwidth (read + write of 1 GiB), the practical ceiling beside the 8 TB/s spec
        src_buf = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
        dst_buf = torch.empty_like(src_buf)
        dst_buf.copy_(src_buf); torch.cuda.synchronize()
        tc = time.perf_counter()
        for _ in range(5):
            dst_buf.copy_(src_buf)
        torch.cuda.synchronize()
        copy_gbps = 5 * 2 * (1 << 30) / (time.perf_counter() - tc) / 1e9
        del src_buf, dst_buf
        # HBM bytes per pass from the PMC counters (collected in separate rocprofv3 --pmc passes and
        # committed under profiles/; valid only for the workload/batch/mode they were taken on)
        # (a counter set counts only when it was taken on THIS device code -- describe()'s hash of the kernel sources, or the compile-time
        # stamp for sets that predate the hash -- otherwise null)
        build_stamp, src_hash = dec.describe().get("build"), dec.describe().get("kernel_sources")

        def same_code(t):
            return (src_hash is not None and t.get("kernel_sources") == src_hash) or t.get("build") == build_stamp
        traffic = None
        for f in sorted((ROOT / "profiles").glob("*pmc_traffic*.json"), reverse=True):
            t = json.loads(f.read_text())
            if same_code(t) and t.get("workload") == args.workload and t.get("batch") == B and t.get("mode") == args.mode and t.get("message_bytes", 1) == b_msg:
                traffic = t.get("fused_pass_hbm_bytes_per_launch" if fu["launches"] else "resident_hbm_bytes_per_launch" if prof.get("resident", {}).get("launches") else "vn_pass_hbm_bytes_per_pass")
                break
        # what limits the dominant kernel on the chip besides HBM (SQ counters collected by tools/profile_round.sh in their own
        # rocprofv3 --pmc passes, summarised by tools/pmc_limiter.py and committed under profiles/; same validity rule)
        limiter = None
        for f in sorted((ROOT / "profiles").glob("*pmc_limiter*.json"), reverse=True):
            t = json.loads(f.read_text())
            if same_code(t) and t.get("workload") == args.workload and t.get("batch") == B and t.get("mode") == args.mode:
                limiter = {"valu_busy": t["valu_busy"], "lds_busy": t["lds_busy"],
                           "lds_bank_conflict_share_of_lds_cycles": t["lds_bank_conflict_share_of_lds_cycles"],
                           "hbm_share_of_achievable_6p3TBps": None, "source": f.name,
                           "note": "shares of the launch during which the vector ALUs issue / the LDS is busy (rocprofv3 --pmc)"}
                break
        if fu["launches"]:
            # skewed two-half pipeline: one decode = 2*I launches of pass_fused_kernel which together carry the
            # I check passes and I-1 variable passes of every frame (first/last launch work on one half only)
            fu_bytes = (I * cn_bytes + (I - 1) * vn_bytes) / (2 * I)
            # as-shipped mode: bytes of the iterations the frames actually executed, spread over the same 2*I launches
            # (late launches carry fewer frames; a finished frame that still rides along in its group is NOT counted)
            fu_bytes *= it_eff / I
            # chain fusion (degree-2 variable nodes updated inside the check pass: dual-diagonal codes) removes one write
            # and one read of two rows per such node and iteration from the launches -- the bytes below stay the canonical
            # algorithmic ones of SURVEY 8(d), `traffic` (PMC) shows what the fused design really moves
            n_chain = int(dec.describe().get("chain_nodes", 0)) if not psc else 0
            saved = n_chain * 4 * 256 * (B / dec.describe()["tile_frames"]) * (I - 1) / (2 * I)
            roof = {"bound": "hbm", "kernel": "pass_fused_kernel (check pass of one half-batch + variable pass of the other)",
                    "achieved": fu_bytes / (fu_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                    "frac": fu_bytes / (fu_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, "traffic": traffic,
                    "algorithmic_bytes_per_launch": fu_bytes, "avg_launch_ms": fu_ms, "launches": fu["launches"],
                    "bytes_not_moved_thanks_to_chain_fusion_per_launch": saved,
                    "achieved_after_fusion_GBps": (fu_bytes - saved) / (fu_ms * 1e-3) / 1e9,
                    # the HBM utilisation proper: bytes really moved (PMC traffic of this build when there is one, else canonical - fused)
                    "frac_of_bytes_moved": (traffic if traffic else fu_bytes - saved) / (fu_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS}
            if limiter is not None:
                limiter["hbm_share_of_achievable_6p3TBps"] = ((traffic if traffic else fu_bytes - saved) / (fu_ms * 1e-3) / 1e9) / 6300.0
                roof["limiter"] = limiter
        elif prof.get("resident", {}).get("launches"):
            rs_ms = prof["resident"]["ms"] / prof["resident"]["launches"]
            bpf = algorithmic_bytes_per_frame(E, N, it_eff, b_msg)
            roof = {"bound": "hbm", "kernel": KERNEL_OF_KIND["resident"], "achieved": bpf * B / (rs_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                    "frac": bpf * B / (rs_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, "traffic": traffic, "algorithmic_bytes_per_launch": bpf * B, "avg_launch_ms": rs_ms,
                    "launches": prof["resident"]["launches"],
                    "note": "messages stay in LDS for the whole decode: the launch moves only labels in and bits out through HBM; the fraction prices the canonical SURVEY 8(d) bytes"}
        else:
            roof = {"bound": "hbm", "kernel": "vn_pass", "achieved": vn_bytes / (vn_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBPS,
                    "unit": "GB/s", "frac": vn_bytes / (vn_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, "traffic": traffic,
                    "algorithmic_bytes_per_launch": vn_bytes, "avg_launch_ms": vn_ms, "launches": vn["launches"]}
        result.update({
            "roofline": roof,
            "roofline_cn_pass": None if not cn["launches"] else {
                "bound": "hbm", "achieved": cn_bytes / (cn_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                "frac": cn_bytes / (cn_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, "algorithmic_bytes_per_launch": cn_bytes,
                "avg_launch_ms": cn_ms, "launches": cn["launches"]},
            # bytes = 4 I E b + (I+2) N b + N/8 with I = iterations actually executed (as-shipped mode: the mean)
            "roofline_whole_decode": {"algorithmic_bytes_per_frame": (4 * it_eff * E + (it_eff + 2) * N) * b_msg + N / 8,
                                      "achieved_GBps": ((4 * it_eff * E + (it_eff + 2) * N) * b_msg + N / 8) * value / world / 1e9,
                                      "bytes_per_label": b_msg, "iterations_counted": it_eff,
                                      "device_copy_GBps_measured": copy_gbps},
            "kernel_ms_per_step": {k: v["ms"] / args.steps for k, v in prof.items() if v["launches"]},
            "single_steps": step_stats,
            "ms_per_step_instrumented": None if args.no_kernel_events else dt_instr / args.steps * 1e3,
        })
        if args.frame_loop_steps > 0:
            # The whole frame loop of LDPC_BER_Sim::sim_snr_point (src/LDPC_BER_Sim.cpp:260-291) on the device:
            # channel sampler -> decode -> error counting, labels never leave HBM.  Reported beside `value`
            # (which stays the decode throughput on resident labels), not instead of it.
            cd.sim_batch(snr, 99, 0, 0, B)
            dec.set_profiling(True); dec.reset_profile()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for k in range(args.frame_loop_steps):
                st = cd.sim_batch(snr, 99, 0, (k + 1) * B, B)
            t_loop = time.perf_counter() - t1
            pf = dec.profile(); dec.set_profiling(False)
            result["frame_loop"] = {"codewords_per_s_per_gpu": B * args.frame_loop_steps / t_loop, "steps": args.frame_loop_steps,
                                    "frontend_ms_per_step": pf["frontend"]["ms"] / args.frame_loop_steps,
                                    "frame_errors_last_step": int((st[:, 1] != 0).sum()),
                                    "note": "device sampler (Philox4x32-10 cell sampler) + decode + BER/FER counting, zero codeword"}
            if world == 1:
                # the same loop as the C++ ber_sim drives it (ber_sim_multi.cpp, default two lanes per device): two simulation objects with
                # their own decoder handle and stream on two host threads -- while one lane's decode occupies the device the other lane's
                # sampler runs and its counters travel back; frames are Philox-addressed, the lanes take alternate batches
                import threading
                cd2 = L.Codec(ROOT / "data" / "codes" / f"{alist}.alist", known_rank=known_rank, device=local)
                cd2.design_luts(sigma2=sigma * sigma, max_iters=max_iter, nq_cha=1 << qc, nq_msg=1 << qm, **extra)
                cd2.set_exit_conditions(max_iter, psc, psc)
                if qcha_map is not None:
                    cd2.set_initial_message_mode(1)
                lanes = [cd, cd2]
                for ln in lanes:
                    ln.sim_batch(snr, 99, 0, 0, B)
                per_lane = args.frame_loop_steps

                def lane(i):
                    for k in range(per_lane):
                        lanes[i].sim_batch(snr, 99, 0, (1 + 2 * k + i) * B, B)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                th = [threading.Thread(target=lane, args=(i,)) for i in range(2)]
                for t_ in th:
                    t_.start()
                for t_ in th:
                    t_.join()
                t_two = time.perf_counter() - t1
                result["frame_loop"]["two_lanes_codewords_per_s_per_gpu"] = 2 * per_lane * B / t_two
                cd2.close()
        if args.as_shipped_steps > 0 and not psc:
            # The reference's default mode (parity_check_iter = true: exit test every iteration, src/LDPC_BER_Sim.cpp:71,500) on
            # frames 0.4 dB above the design point, where they converge: reported beside `value`, never instead of it.
            snr_s = snr + 0.4
            cha_s, msg_s = make_labels_device(cd, B, snr_s, seed=4321 + rank, qcha_map=qcha_map)
            cd.set_exit_conditions(max_iter, True, True)
            it_s = torch.empty(B, dtype=torch.int32, device="cuda")
            bits_s = torch.empty_like(out_bits)                    # (out_bits / out_iters still hold the fixed-work result the oracle checks)

            def step_s(sync):
                dec.lut_decode_batch_device(cha_s.data_ptr(), msg_s.data_ptr(), B, bits_s.data_ptr(), it_s.data_ptr(), sync=sync)
            torch.cuda.synchronize()                               # the labels are written on torch's stream, the decoder runs on its own
            step_s(True); step_s(True)
            if os.environ.get("BENCH_DEBUG"):
                print("debug as_shipped warm", float(it_s.abs().float().mean().item()), int((it_s < 0).sum().item()), int(cha_s.sum(dtype=torch.int64).item()), int(msg_s.sum(dtype=torch.int64).item()), file=sys.stderr)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for k in range(args.as_shipped_steps):
                step_s(k == args.as_shipped_steps - 1)
            torch.cuda.synchronize()
            t_s = time.perf_counter() - t1
            result["as_shipped"] = {"codewords_per_s_per_gpu": B * args.as_shipped_steps / t_s, "steps": args.as_shipped_steps,
                                    "EbN0_dB": float(snr_s), "mean_iterations_executed": float(it_s.abs().float().mean().item()),
                                    "frames_that_left_through_the_exit_test": int((it_s > 0).sum().item()),
                                    "note": "parity_check_iter = true (exit test every iteration, finished frames retired by compaction), "
                                            "same decoder, labels resident in HBM"}
            if rank == 0 and not args.no_cpu_baseline:
                # the as-shipped result against the oracle under psc = pisc = 1: a sample over every kind of outcome, from the
                # whole batch (this is the path every batch of BASELINE config 4 takes: chain fusion + compaction + late decided bits)
                it_h = it_s.cpu().numpy()
                idx = outcome_sample(it_h, 64, max_iter)
                sel = torch.from_numpy(idx).cuda()
                oc = oracle_codec_for(cd, max_iter, True, True)
                t1 = time.perf_counter()
                wb, wi = oc.lut_decode_batch_flat(cha_s[sel].cpu().numpy(), msg_s[sel].cpu().numpy(), threads=usable_cores())
                same = bool((wi == it_h[idx]).all() and (wb == bits_s[sel].cpu().numpy()).all())
                result["as_shipped"].update({"gpu_matches_oracle_on_sample": same, "frames_compared_with_oracle": int(len(idx)),
                                             "sample_outcomes": {"failed": int((wi < 0).sum()), "passed_on_channel_decisions": int((wi == 0).sum()),
                                                                 "early_exit": int(((wi > 0) & (wi < max_iter)).sum()), "full_count": int((wi == max_iter).sum())},
                                             "oracle_s": time.perf_counter() - t1, "compaction_active": bool(0 < dec.describe().get("compaction_min_groups", -1) <= (B + dec.describe()["tile_frames"] - 1) // dec.describe()["tile_frames"])})
                if not same:
                    raise SystemExit("as-shipped GPU output differs from the oracle on the sample")
            cd.set_exit_conditions(max_iter, psc, psc)
            del cha_s, msg_s, bits_s
        configs = None
        if rank == 0 and world == 1 and args.workload == "dvbs2" and not args.no_configs:
            # the headline decoder's buffers (7 GB at 32768 frames) go first; its outputs are kept for the oracle check below
            keep_bits, keep_iters = out_bits[:n_host].cpu().numpy(), out_iters[:n_host].cpu().numpy()
            configs = {}
            for wl, Bc in (("c2", 4096), ("c5", 36864), ("c5chk", 32768), ("c1", 16384), ("twin", 32768)):
                configs[wl] = quick_config(L, torch, wl, Bc, local)
        result["configs"] = configs
        if rank == 0 and world == 1 and not args.no_cpu_baseline:
            base, ob, oi, fb, fi = cpu_baseline(cd, cha_h, msg_h, max_iter, psc)
            n, nf = len(oi), len(fi)
            same = bool((ob == out_bits[:n].cpu().numpy()).all() and (oi == out_iters[:n].cpu().numpy()).all()
                        and (fb == out_bits[:nf].cpu().numpy()).all() and (fi == out_iters[:nf].cpu().numpy()).all())
            base["gpu_matches_oracle_on_sample"] = same
            base["frames_compared_with_gpu"] = int(max(n, nf))
            result["cpu_baseline"] = base
            if not same:
                raise SystemExit("GPU output differs from the oracle on the cpu_baseline sample")
        elif rank == 0:
            result["cpu_baseline"] = None
    if rank == 0:
        print(json.dumps(result))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()