"""Cases and references of the packed device encoder (lutldpc_decoder_encode_packed), shared by tests/test_encode_packed_cpu.py (checks
that the lists hold what they claim and the references against the oracle, without a GPU) and tests/test_58_encode_packed_gpu.py
(holds the kernel to the references through the C-ABI).  The references are plain numpy: frontend_cases.encode is the statement of
[u | A u mod 2] for the synthetic generators, a GF(2) elimination of the parity-check matrix is the one for the real codes.  All
integer, equal bit for bit."""
from __future__ import annotations

import functools

import numpy as np

import frontend_cases as fc

# ---------------------------------------------------------------------------------------------------------------- bit order
SHIFTS = np.arange(32, dtype=np.uint32)


def pack(bits):
    """bits[B, n] of 0 / 1 -> uint32[B, ceil(n/32)]: bit j of word w = bit 32w + j, spare bits 0 (written here on its own, not with the
    product's packing.pack_bits, which the CPU test holds against this one)."""
    bits = np.asarray(bits, np.uint8)
    B, n = bits.shape
    padded = np.zeros((B, (n + 31) // 32 * 32), np.uint8)
    padded[:, :n] = bits
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u4").astype(np.uint32).reshape(B, -1)


def unpack(words, n):
    """uint32[B, W] -> uint8[B, n], the first n bits in that order."""
    words = np.ascontiguousarray(words, np.uint32)
    return ((words[:, :, None] >> SHIFTS[None, None, :]) & np.uint32(1)).reshape(len(words), -1)[:, :n].astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- synthetic generators
# (handle of frontend_cases.HANDLES, K, R): the raw lutldpc_decoder_set_generator with frontend_cases.generator_rows (random in all 64
# bits of every word: bits beyond K are set).  K = 1000 has no parity at all, (8192, 1808) is the LDS limit of the kernel.
SYNTH_CASES = [(h, K, 1000 - K) for h in ("q4", "q4_pack1") for K in (1, 31, 32, 33, 127, 128, 129, 500, 968, 999, 1000)] + \
              [("n127", 64, 63), ("n10000", 8192, 1808)]
BATCHES = (1, 63, 64, 65, 130)                      # the 64-frame workgroup at, under and over its edge
SPARE_WORDS = 3                                     # the second frame stride: ceil(K/32) + 3 words, the spare ones random
GUARD_WORDS = 4                                     # behind the last frame of the output
FILL = 0xEE


def synth_id(case):
    return f"{case[0]}-K{case[1]}-R{case[2]}"


def windows(K, R):
    """The (first, count) windows of codeword bits of a case, in a fixed order and without repeats."""
    N = K + R
    out = [(0, N), (0, K)]
    if R > 0:
        out.append((K, R))
    out += [(K - 1, min(34, N - K + 1)), (31, 66), (N - 1, 1)]
    rng = np.random.default_rng(K * 31 + R)
    for _ in range(3):
        first = int(rng.integers(0, N))
        out.append((first, int(rng.integers(1, N - first + 1))))
    assert all(f >= 0 and c >= 1 and f + c <= N for f, c in out), (K, R, out)
    return list(dict.fromkeys(out))


@functools.lru_cache(maxsize=None)
def info_words(K, stride):
    """[max(BATCHES), stride] uint32, random in all 32 bits of every word: the bits beyond K of the last word and the spare words
    behind it are set and must be ignored.  A smaller batch is a prefix.  Read-only."""
    w = np.random.default_rng(K * 7919 + stride).integers(0, 1 << 32, (max(BATCHES), stride), dtype=np.uint32)
    w.setflags(write=False)
    return w


def strides(K):
    """(in_stride given to the entry, words per frame of the buffer)"""
    W = (K + 31) // 32
    return [(0, W), (W + SPARE_WORDS, W + SPARE_WORDS)]


@functools.lru_cache(maxsize=None)
def synth_generator(K, R):
    A = fc.generator_bits(fc.generator_rows(K, R), K)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def synth_reference(K, R, stride):
    """The codewords uint8 [max(BATCHES), K + R] of info_words(K, stride): the masked information bits and A u mod 2."""
    u = unpack(info_words(K, stride)[:, :(K + 31) // 32], K)
    cw = fc.encode(synth_generator(K, R), u).astype(np.uint8)
    cw.setflags(write=False)
    return cw


def window_words(cw, first, count):
    """What the entry returns for codewords cw[B, N] and a window."""
    return pack(cw[:, first:first + count])


# ---------------------------------------------------------------------------------------------------------------- real codes
# name -> (alist, design of the product codec); N2048 with the trees of 6_32_wide.ini has rank 325 < nchk = 384
REAL_CODES = {
    "N500": ("rate0.50_dv02-17_dc08-09_lut_q4_N500", dict(sigma2=0.88 ** 2, max_iters=4)),
    "N1000": ("rate0.50_dv03_dc06_N1000", dict(sigma2=0.88 ** 2, max_iters=4)),
    "N2048": ("rate0.84_reg_v6c32_N2048", dict(tree="6_32_wide.ini", design_snr_db=3.9, max_iters=8, nq_cha=16, nq_msg=8)),
}
REAL_B = 130


def product_codec(name, device):
    """The product's Codec of a real code, with its generator (device = -1: host only)."""
    import lut_ldpc_amd as L
    from helpers import CODES, TREES
    alist, kw = REAL_CODES[name]
    kw = dict(kw)
    pcd = L.Codec(CODES / f"{alist}.alist", with_generator=True, device=device)
    tree = kw.pop("tree", None)
    if tree:
        snr = kw.pop("design_snr_db")
        kw.update(tree_method="filename=" + str(TREES / tree), sigma2=10 ** (-snr / 10) / (2 * (1.0 - pcd.rank / pcd.nvar)))
    pcd.design_luts(**kw)
    return pcd


def parity_check_matrix(nvar, nchk, dv, dc, cn_msg_idx):
    """H uint8 [nchk, nvar] from the graph arrays of the C-ABI: cn_msg_idx lists, check by check, the variable-major edge ids."""
    var_of_edge = np.repeat(np.arange(nvar), dv)
    chk_of_slot = np.repeat(np.arange(nchk), dc)
    H = np.zeros((nchk, nvar), np.uint8)
    np.add.at(H, (chk_of_slot, var_of_edge[cn_msg_idx]), 1)
    return H & 1


def systematic_rows(H, K):
    """A uint8 [N - K, K] with parity = A u mod 2 for H = [Hu | Hp], Hp = the last N - K columns (of full column rank): Gauss-Jordan
    over GF(2) on [Hp | Hu].  Rows without a pivot must vanish, or H would constrain the information bits."""
    M, N = H.shape
    R = N - K
    T = np.concatenate([H[:, K:], H[:, :K]], axis=1).astype(bool)
    for i in range(R):
        p = i + int(np.argmax(T[i:, i]))
        assert T[p, i], ("parity column without a pivot", i)
        if p != i:
            T[[i, p]] = T[[p, i]]
        rows = np.flatnonzero(T[:, i])
        rows = rows[rows != i]
        T[rows] ^= T[i]
    assert not T[R:].any() and (T[:R, :R] == np.eye(R, dtype=bool)).all()
    return T[:R, R:].astype(np.uint8)


@functools.lru_cache(maxsize=None)
def real_reference(name):
    """dict of a real code: N, K, R, the graph, the data words [REAL_B, ceil(K/32)] (random in all 32 bits) and the reference's
    codewords uint8 [REAL_B, N] -- from the graph the product's host code hands out (its column order) by elimination in numpy."""
    pcd = product_codec(name, device=-1)
    N, K, R = pcd.nvar, pcd.ninfo, pcd.rank
    graph = (N, pcd.nchk) + tuple(pcd.graph())
    pcd.close()
    A = systematic_rows(parity_check_matrix(*graph), K)
    words = np.random.default_rng(N).integers(0, 1 << 32, (REAL_B, (K + 31) // 32), dtype=np.uint32)
    cw = fc.encode(A, unpack(words, K)).astype(np.uint8)
    for a in (words, cw):
        a.setflags(write=False)
    return dict(N=N, K=K, R=R, graph=graph, words=words, cw=cw)


# ---------------------------------------------------------------------------------------------------------------- loop-back
LOOP_CODE, LOOP_B = "N1000", 130


def loop_llr_magnitude(qb_cha):
    """L beyond the top boundary of qb_cha (and -L below the bottom one): twice the largest magnitude plus one."""
    return 2.0 * float(np.max(np.abs(qb_cha))) + 1.0


@functools.lru_cache(maxsize=None)
def loop_reference():
    """The loop-back case with the oracle alone: the codewords of real_reference(LOOP_CODE) sent as LLR = +-L (float32), quantised
    and decoded by the oracle with psc on.  dict: L, the data words, the decided data words and the iteration codes."""
    from helpers import design
    from oracle import oracle as orc
    ref = real_reference(LOOP_CODE)
    kw = REAL_CODES[LOOP_CODE][1]
    oc = design(orc.Code(graph=ref["graph"]), ref["R"], kw["sigma2"], kw["max_iters"], 16, nq_cha=16)
    oc.set_exit_conditions(kw["max_iters"], True, False)
    L = loop_llr_magnitude(oc.qb_cha)
    llr = (L * (1.0 - 2.0 * ref["cw"])).astype(np.float32)
    cha, msg = orc.quant_nonlin(llr.astype(np.float64), oc.qb_cha), orc.quant_nonlin(llr.astype(np.float64), oc.qb_msg)
    bits, iters = oc.lut_decode_batch(cha, msg)
    return dict(L=L, words=ref["words"], decided=pack(bits[:, :ref["K"]]), iters=iters, cha=cha, nq_cha=16, qb_cha=oc.qb_cha, max_iters=kw["max_iters"])
