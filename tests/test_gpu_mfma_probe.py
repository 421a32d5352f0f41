"""ds_read_b64_tr_b16 lane mapping, checked on the hardware.

Every transposed MFMA fragment (frag_tr in csrc/mfma_frag.h: attention
PV/dQ/dK/dV, wgrad) assumes one rule for the hardware transpose read:
within each 16-lane group, with lane numbers relative to the group,

    out[lane i][j] = mem[addr_of_lane(4*j + (i >> 2)) + (i & 3)]

tr16_probe (csrc/ops/mfma_probe.hip) fills LDS with mem[k] = k, gives
lane t the element offset addr_of_lane(t) of its addr_mode and returns
what each lane's four slots received. Modes 0 and 2 are the address
patterns frag_tr produces. @pytest.mark.gpu."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bert_pytorch_amd import ops


def addr_of_lane(mode: int) -> np.ndarray:
    """Element offset each of the 64 lanes passes, as in the kernel's
    switch on addr_mode."""
    t = np.arange(64)
    if mode == 0:
        return t * 4              # 8 B per lane, contiguous
    if mode == 1:
        return np.zeros(64, int)  # uniform base
    if mode == 2:
        return (t & 15) * 4       # repeats per 16-lane group
    return (t >> 4) * 4           # group-constant


def expected(mode: int) -> np.ndarray:
    addr = addr_of_lane(mode)
    out = np.empty((64, 4), dtype=np.float32)
    for lane in range(64):
        group, i = lane & ~15, lane & 15
        for j in range(4):
            src = group + 4 * j + (i >> 2)
            out[lane, j] = addr[src] + (i & 3)
    return out


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_tr16_probe_matches_documented_rule(mode):
    got = ops.extension().tr16_probe(mode)
    assert got.shape == (64, 4) and got.dtype == torch.float32
    np.testing.assert_array_equal(got.cpu().numpy(), expected(mode))
