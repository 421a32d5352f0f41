"""The dropout RNG on CPU: the numpy Philox of philox_ref.py against the
Random123 known-answer vectors, and the counter reservations of
ops.rng.next_philox against what each kernel consumes."""

import numpy as np
import pytest

import philox_ref
from bert_pytorch_amd.ops import rng


# Random123 kat_vectors, philox4x32 with 10 rounds: counter, key, expected
_KAT = [
    ((0, 0, 0, 0), (0, 0),
     (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2,
     (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344),
     (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", _KAT)
def test_philox_known_answers(ctr, key, want):
    got = philox_ref.philox4x32_10_words(*ctr, *key)
    assert [int(w) for w in got] == list(want)


def test_philox_counter_and_seed_halves():
    """The 2-argument form puts the counter in (c0, c1), zeros in (c2, c3)
    and the seed halves in (k0, k1): equal to the 4-word form so fed, for
    values that use the high halves, and vectorised over counters."""
    seed = (1 << 40) + 12345
    ctrs = np.array([0, 7, (1 << 32) - 1, 1 << 32, (1 << 33) + 1],
                    dtype=np.uint64)
    got = philox_ref.philox4x32_10(ctrs, seed)
    assert got.shape == (5, 4) and got.dtype == np.uint32
    for i, c in enumerate(int(c) for c in ctrs):
        want = philox_ref.philox4x32_10_words(
            c & 0xFFFFFFFF, c >> 32, 0, 0, seed & 0xFFFFFFFF, seed >> 32
        )
        assert (got[i] == want).all()
    # the first vector again through the 2-argument form
    assert [int(w) for w in philox_ref.philox4x32_10(0, 0)] == list(_KAT[0][2])
    # high halves matter: c1 and k1 change the output
    assert (got[2] != got[3]).any()
    assert (philox_ref.philox4x32_10(7, seed)
            != philox_ref.philox4x32_10(7, seed & 0xFFFFFFFF)).any()


def test_keep_mask_layout():
    """bdrl_keep_mask: element e is word e % 4 of counter offset + e // 4;
    a mask that starts 4 elements later is the same stream one counter on,
    also across the carry into the counter's high word."""
    seed, off = 5, (1 << 32) - 3
    a = philox_ref.bdrl_keep_mask(3, 16, 0.5, seed, off).reshape(-1)
    b = philox_ref.bdrl_keep_mask(3, 16, 0.5, seed, off + 1).reshape(-1)
    assert (a[4:] == b[:-4]).all()
    r = philox_ref.philox4x32_10(off + 5, seed)
    want = (r.astype(np.float64) / 2.0 ** 32 >= 0.5).astype(np.uint8)
    assert (a[20:24] == want).all()
    assert 0 < a.sum() < a.size


def test_attention_bits_layout():
    """attention_keep_bits: S = 48 pads each row to two words; bit j of
    word i is byte j & 3 of output j >> 2 of counters offset + 2i (+1)."""
    seed, off, p = (1 << 40) + 12345, 7, 0.1
    bits = philox_ref.attention_keep_bits(2, 48, p, seed, off)
    assert bits.shape == (2, 48, 2) and bits.dtype == np.int32
    flat = bits.reshape(-1).view(np.uint32)
    i = 37
    r = np.concatenate([philox_ref.philox4x32_10(off + 2 * i, seed),
                        philox_ref.philox4x32_10(off + 2 * i + 1, seed)])
    for j in (0, 3, 4, 17, 31):
        byte = (int(r[j >> 2]) >> (8 * (j & 3))) & 0xFF
        assert ((int(flat[i]) >> j) & 1) == (1 if byte >= 26 else 0)


def _reserve_chain(calls):
    """Run next_philox over (n_elements, consumed) calls; return the
    (base, consumed) pairs."""
    rng.reset(1234)
    try:
        return [(rng.next_philox(n)[1], used) for n, used in calls]
    finally:
        rng.reset()


def test_reservations_cover_consumption():
    """No kernel's counters reach the next caller's base offset. bdrl and
    the embedding kernel consume ceil(rows*H/4) counters of a
    next_philox(rows*H) reservation; the attention mask consumes
    2*B*NH*S*ceil(S/32) of next_philox(B*NH*S*S)."""
    calls = []
    for rows in (1, 3, 37, 87, 512, 4096 * 3):
        for H in (64, 768, 1024, 2056, 4096):
            calls.append((rows * H, philox_ref.bdrl_counters_consumed(rows, H)))
    # S: the attention kernels take multiples of 16 (padded) and any
    # max_seqlen rounded likewise (packed); 16..512 with non-multiples of 32
    for S in (16, 32, 48, 80, 112, 128, 144, 368, 384, 496, 512):
        for B, NH in ((1, 1), (1, 2), (3, 12), (8, 16), (64, 16)):
            calls.append(
                (B * NH * S * S,
                 philox_ref.attention_counters_consumed(B, NH, S))
            )
    chain = _reserve_chain(calls)
    for (base, used), (next_base, _) in zip(chain, chain[1:]):
        assert used > 0
        assert base + used <= next_base, (base, used, next_base)
    # and the helpers state what the kernels do
    assert philox_ref.bdrl_counters_consumed(37, 64) == 592
    assert philox_ref.attention_counters_consumed(1, 2, 48) == 2 * 2 * 48 * 2


def test_seed_is_64_bit_clean():
    """next_philox hands the seed on as a non-negative int64 (the binding
    takes int64_t), wide seeds included."""
    rng.reset((1 << 40) + 12345)
    try:
        seed, base = rng.next_philox(10)
        assert seed == (1 << 40) + 12345 and base == 0
        assert rng.next_philox(10)[1] == 4  # ceil(10/4) + 1
    finally:
        rng.reset()
