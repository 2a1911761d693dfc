"""The zero-cell footprint of SOC_BLOOM_SPARSE (bloom_w.hpp zero_cell_footprint, the host side of the kernels' proof).

The weighted chain's output is a function of mip3 alone (mip3 -> mip2 -> mip1 -> mip0 -> output, every upsample
overwriting its target). The sparse last stage and Composition treat a 32 x 16 output cell as exactly zero when the mip3
texels of the cell's footprint are: the footprint must therefore hold every mip3 texel that reaches the cell. Checked
with a one-texel impulse at every mip3 position through the CPU oracle's upsample (no GPU): every non-zero output pixel
lies in a cell whose footprint holds the impulse (sufficient), and every offset of the declared range is attained
(tight). 128 x 64: whole cells; 200 x 72: a partial last cell column and row, mip3 25 x 9."""
import numpy as np
import pytest

from helpers import globals_for

CELL_W, CELL_H = 32, 16


def upsweep(oracle, g, mip3, W, H):
    """mip3 -> output through the four upsamples of the chain."""
    lo = mip3
    for w, h in ((W // 4, H // 4), (W // 2, H // 2), (W, H), (W, H)):
        hi = np.zeros((h, w, 4), np.float16)
        oracle.bloom_upsample(g, lo, hi)
        lo = hi
    return lo


def test_footprint_values(soc):
    """Columns clamp(4a - 3 .. 4a + 6), rows clamp(2b - 3 .. 2b + 4)."""
    assert soc.bloom_zero_cell_footprint(0, 0, 16, 8) == (0, 6, 0, 4)
    assert soc.bloom_zero_cell_footprint(2, 1, 16, 8) == (5, 14, 0, 6)
    assert soc.bloom_zero_cell_footprint(3, 3, 16, 8) == (9, 15, 3, 7)
    assert soc.bloom_zero_cell_footprint(6, 4, 25, 9) == (21, 24, 5, 8)


@pytest.mark.parametrize("W,H", [(128, 64), (200, 72)])
def test_impulse_stays_inside_the_footprint(soc, oracle, W, H):
    g = globals_for(W, H)
    w3, h3 = W // 8, H // 8
    ncx, ncy = -(-W // CELL_W), -(-H // CELL_H)
    foot = {(a, b): soc.bloom_zero_cell_footprint(a, b, w3, h3) for a in range(ncx) for b in range(ncy)}
    dxs, dys = set(), set()
    for y3 in range(h3):
        for x3 in range(w3):
            mip3 = np.zeros((h3, w3, 4), np.float16)
            mip3[..., 3] = 1.0
            mip3[y3, x3, :3] = 4096.0   # the smallest path weight is 2^-24: still a normal RGBA16F value
            out = upsweep(oracle, g, mip3, W, H)
            ys, xs = np.nonzero((out[..., :3].view(np.uint16) != 0).any(axis=2))
            assert len(xs), (x3, y3)
            for a, b in {(int(x) // CELL_W, int(y) // CELL_H) for x, y in zip(xs, ys)}:
                x0, x1, y0, y1 = foot[(a, b)]
                assert x0 <= x3 <= x1 and y0 <= y3 <= y1, ((x3, y3), (a, b), foot[(a, b)])
                dxs.add(x3 - 4 * a)
                dys.add(y3 - 2 * b)
    assert dxs == set(range(-3, 7)) and dys == set(range(-3, 5)), (sorted(dxs), sorted(dys))
