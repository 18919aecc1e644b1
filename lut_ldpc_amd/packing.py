"""Host-side formats of Decoder.decode_packed (lutldpc_decoder_decode_batch_packed, include/lut_ldpc_hip.h): labels two per byte
going in, decided bits one per bit coming out -- and of Decoder.encode_packed, which takes and returns bits in that bit format.
Plain numpy, no device.

Nibble format (LUTLDPC_IN_NIBBLES): frame stride ceil(N/2) bytes, node v in byte v // 2, even v in bits 0-3, odd v in bits 4-7;
the spare nibble of an odd N is written as 0 here and ignored by the decoder.
Bit format: words[B, ceil(count/32)] uint32, bit j of word w = bit 32w + j of the window; bits beyond count are 0.
"""
from __future__ import annotations

import numpy as np


def pack_nibbles(labels) -> np.ndarray:
    """labels[B, N] with values below 16 -> uint8[B, ceil(N/2)]."""
    labels = np.asarray(labels)
    if labels.ndim != 2:
        raise ValueError("labels must be [B, N]")
    if labels.size and (labels.min() < 0 or labels.max() > 15):
        raise ValueError("a nibble holds labels 0..15")
    B, N = labels.shape
    even = np.zeros((B, (N + 1) // 2), np.uint8)
    odd = np.zeros_like(even)
    even[:, :] = labels[:, 0::2]
    odd[:, :N // 2] = labels[:, 1::2]
    return even | (odd << 4)


def unpack_nibbles(packed, N: int) -> np.ndarray:
    """uint8[B, ceil(N/2)] -> labels uint8[B, N]; the spare nibble of an odd N is dropped."""
    packed = np.asarray(packed, np.uint8)
    if packed.ndim != 2 or packed.shape[1] != (N + 1) // 2:
        raise ValueError("packed must be [B, ceil(N/2)]")
    out = np.empty((packed.shape[0], 2 * packed.shape[1]), np.uint8)
    out[:, 0::2] = packed & 0x0F
    out[:, 1::2] = packed >> 4
    return np.ascontiguousarray(out[:, :N])


def unpack_bits(words, count: int) -> np.ndarray:
    """words[B, W] uint32 with W >= ceil(count/32) -> uint8[B, count] of 0 / 1."""
    words = np.ascontiguousarray(words, np.uint32)
    if words.ndim != 2 or 32 * words.shape[1] < count:
        raise ValueError("words must be [B, W] with 32 * W >= count")
    shifts = np.arange(32, dtype=np.uint32)
    bits = (words[:, :, None] >> shifts[None, None, :]) & np.uint32(1)
    return np.ascontiguousarray(bits.reshape(words.shape[0], -1)[:, :count].astype(np.uint8))


def pack_bits(bits) -> np.ndarray:
    """bits[B, n] of 0 / 1 -> uint32[B, ceil(n/32)], the inverse of unpack_bits: bit j of word w = bit 32w + j, the spare bits of the
    last word are 0.  The input format of Decoder.encode_packed."""
    bits = np.asarray(bits)
    if bits.ndim != 2:
        raise ValueError("bits must be [B, n]")
    if bits.size and (bits.min() < 0 or bits.max() > 1):
        raise ValueError("bits must be 0 or 1")
    B, n = bits.shape
    padded = np.zeros((B, (n + 31) // 32 * 32), np.uint32)
    padded[:, :n] = bits
    shifts = np.arange(32, dtype=np.uint32)
    return np.ascontiguousarray((padded.reshape(B, -1, 32) << shifts[None, None, :]).sum(axis=2, dtype=np.uint32))
