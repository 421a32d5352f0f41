"""Numpy Philox4x32-10 and the dropout keep-masks built from it.

Written from ``Philox::operator()`` in csrc/common.h and the mask code of
the kernels that use it, so the GPU tests can compare dropout masks bit
for bit. All arithmetic is uint64 with explicit 32-bit masking; every
function takes scalars or arrays of counters and is vectorised.
"""

from __future__ import annotations

import numpy as np

_M0 = np.uint64(0xD2511F53)
_M1 = np.uint64(0xCD9E8D57)
_W0 = np.uint64(0x9E3779B9)
_W1 = np.uint64(0xBB67AE85)
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10_words(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on a full 4-word counter and 2-word key.

    Arguments are integers or arrays of 32-bit values; returns a uint32
    array of shape ``broadcast(...) + (4,)``.
    """
    c0, c1, c2, c3, k0, k1 = (
        np.asarray(v, dtype=np.uint64) & _LO for v in (c0, c1, c2, c3, k0, k1)
    )
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(c0, c1, c2, c3, k0, k1)
    for _ in range(10):
        p0 = _M0 * c0  # < 2^64: both factors are below 2^32
        p1 = _M1 * c2
        hi0, lo0 = p0 >> _S32, p0 & _LO
        hi1, lo1 = p1 >> _S32, p1 & _LO
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + _W0) & _LO
        k1 = (k1 + _W1) & _LO
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def philox4x32_10(counter_u64, seed_u64):
    """The kernels' use of it: 64-bit counter in (c0, c1), c2 = c3 = 0,
    key = the two halves of the 64-bit seed. Returns ``[..., 4]`` uint32."""
    ctr = np.asarray(counter_u64, dtype=np.uint64)
    seed = np.uint64(int(seed_u64) & 0xFFFFFFFFFFFFFFFF)
    return philox4x32_10_words(
        ctr & _LO, ctr >> _S32, 0, 0, seed & _LO, seed >> _S32
    )


def _counters(offset, n):
    """offset + [0, n) as uint64 (wrapping like the kernel's uint64 add)."""
    with np.errstate(over="ignore"):
        return np.uint64(int(offset)) + np.arange(n, dtype=np.uint64)


def bdrl_keep_mask(rows, H, p, seed, offset):
    """Byte keep-mask [rows, H] of bdrl_fwd_kernel / embed_fwd_kernel:
    element e takes word ``e % 4`` of counter ``offset + e // 4`` and is
    kept when ``float32(u32) * 2^-32 >= float32(p)``. H % 4 == 0."""
    n = rows * H
    assert n % 4 == 0
    r = philox4x32_10(_counters(offset, n // 4), seed).reshape(-1)
    u = r.astype(np.float32) * np.float32(2.0 ** -32)
    return (u >= np.float32(p)).astype(np.uint8).reshape(rows, H)


def attention_keep_bits(BNH, S, p, seed, offset):
    """Bit-packed keep-mask [BNH, S, ceil(S/32)] of dropout_mask_kernel as
    int32 words: word i uses counters ``offset + 2i`` and ``offset + 2i + 1``
    (eight 32-bit outputs); bit j is byte ``j & 3`` of output ``j >> 2``,
    kept when that byte is at least ``round(256 p)`` (capped at 255)."""
    Sw = (S + 31) // 32
    words = BNH * S * Sw
    thresh = min(int(np.floor(p * 256.0 + 0.5)), 255)
    r = philox4x32_10(_counters(offset, 2 * words), seed).reshape(words, 8)
    bits = np.zeros(words, dtype=np.uint32)
    for j in range(32):
        byte = (r[:, j >> 2] >> np.uint32(8 * (j & 3))) & np.uint32(0xFF)
        bits |= (byte >= thresh).astype(np.uint32) << np.uint32(j)
    return bits.view(np.int32).reshape(BNH, S, Sw)


def bdrl_counters_consumed(rows, H):
    """Counters bdrl/embedding dropout consumes from its base offset."""
    return -(-rows * H // 4)


def attention_counters_consumed(B, NH, S):
    """Counters the attention mask kernel consumes from its base offset."""
    return 2 * B * NH * S * ((S + 31) // 32)
