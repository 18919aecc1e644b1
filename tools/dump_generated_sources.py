#!/usr/bin/env python3
"""Write every HIP source the two run-time generators (csrc/hip/jit.hpp, jit_resident.hpp) produce for the configurations of
tests/helpers.py and the codes of tests/streaming_cases.py and tests/resident_cases.py, so that two builds can be compared text by
text (host only, no GPU; the oracle designs the LUTs).
Usage: tools/dump_generated_sources.py OUTDIR [--compile]
OUTDIR/<sha256>.hip holds one distinct text each, OUTDIR/index.txt one line `config kind set class hash` per source: kinds
0 / 1 / 2 / 33 are the streaming pass kernels of Decoder.jit_source (variable, check tree, decision, full-label check tree),
`resident` lines carry the frame groups G and SxNT in the set / class columns (hash `refused`: resident_pick declined).
OUTDIR/describe.txt holds describe() of every configuration without its build stamp and source hash (its "static" section carries
sizes and CRC-32s of the op, table and index blobs), OUTDIR/program_stats.txt one line per (kind, set, class) that answers
Decoder.program_stats, kinds 0 / 1 / 2 and 33.
--compile runs hiprtc (gfx950, the options of jit_compile) on every distinct text and stores OUTDIR/<sha256>.co.
The LUTLDPC_* knobs of the environment apply, LUTLDPC_LIB selects another build: call it once per setting to sweep them."""
import ctypes as C
import hashlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import lut_ldpc_amd as L  # noqa: E402
import resident_cases  # noqa: E402
import streaming_cases  # noqa: E402
from helpers import CONFIGS, oracle_codec, product_decoder  # noqa: E402

out = Path(sys.argv[1])
out.mkdir(parents=True, exist_ok=True)
texts, index, describes, stats = {}, [], [], []
codecs = [(name, oracle_codec) for name in CONFIGS] + [(name, streaming_cases.codec) for name in streaming_cases.CODES] + \
         [(name, resident_cases.codec) for name in resident_cases.LIMITS]


def record(key, src):
    h = hashlib.sha256(src.encode()).hexdigest()
    texts[h] = src
    index.append(f"{key} {h}")


for name, codec in codecs:
    cd = codec(name)
    dec = product_decoder(cd, device=-1)
    desc = {k: v for k, v in dec.describe().items() if k not in ("build", "kernel_sources")}
    describes.append(f"{name} {json.dumps(desc, sort_keys=True)}")
    n_cls = max(len(desc["vn_classes"]), len(desc["cn_classes"]))
    for kind in (0, 1, 2, 33):
        for s in range(cd.n_sets()):
            for cls in range(n_cls):
                try:
                    stats.append(f"{name} {kind} {s} {cls} {json.dumps(dec.program_stats(kind, s, cls), sort_keys=True)}")
                except L.LutLdpcError:
                    pass
    for kind in (0, 1, 2, 33):
        for s in range(cd.n_sets()):
            try:
                for cls in range(1 << 20):
                    record(f"{name} {kind} {s} {cls}", dec.jit_source(kind, s, cls))
            except L.LutLdpcError:      # past the last class, or no program of this kind in this set
                pass
    for G in (1, 2, 3, 8, 64):
        try:
            src, (S, NT, _) = dec.resident_source(G)
            record(f"{name} resident {G} {S}x{NT}", src)
        except L.LutLdpcError:
            index.append(f"{name} resident {G} - refused")
    dec.close()

for h, src in texts.items():
    (out / f"{h}.hip").write_text(src)
for fname, lines in (("index.txt", index), ("describe.txt", describes), ("program_stats.txt", stats)):
    (out / fname).write_text("\n".join(lines) + "\n")
print(f"{len(index)} index entries, {len(texts)} distinct texts, {len(describes)} configurations, {len(stats)} programs")

if "--compile" in sys.argv[2:]:
    rtc = C.CDLL("libhiprtc.so")        # (already loaded: liblut_ldpc_amd.so links it)
    opts = (C.c_char_p * 3)(b"--offload-arch=gfx950", b"-O3", b"-std=c++17")
    for h, src in texts.items():
        prog, n = C.c_void_p(), C.c_size_t()
        assert rtc.hiprtcCreateProgram(C.byref(prog), src.encode(), b"lutldpc_jit_pass.hip", 0, None, None) == 0
        assert rtc.hiprtcCompileProgram(prog, 3, opts) == 0, f"hiprtc failed on {h}"
        assert rtc.hiprtcGetCodeSize(prog, C.byref(n)) == 0
        code = C.create_string_buffer(n.value)
        assert rtc.hiprtcGetCode(prog, code) == 0
        (out / f"{h}.co").write_bytes(code.raw)
        rtc.hiprtcDestroyProgram(C.byref(prog))
    print(f"compiled {len(texts)} texts")
