"""The depth-of-field oracle (tests/dof_oracle.py) on cases whose answer is known without it, and the rounding
sensitivity of the pass's lod on the inputs of the GPU parity test (CPU only).

float64 against float32: evaluating the lod chain (depth -> object distance -> c -> rho -> log2 -> lq) in double moves lq
by at most one 1/256 step anywhere, on this share of the geometry pixels (re-measured with these inputs; cap 2 %):

    64x36  defaults 0.88 %   focus20 1.13 %
    97x55  defaults 0.78 %   focus20 0.93 %
    33x17  defaults 0.82 %   focus20 0.62 %

It is not tighter because the depth-to-distance inversion is ill-conditioned near the far plane: d (far - near) - far
cancels to about near / od of a value near far, so one ulp of the product is 6e-5 against 1e-4 at od = far."""
from fractions import Fraction

import numpy as np
import pytest

import dof_inputs
import dof_oracle
import helpers

F64_CAP = 0.02


def _random_color(H, W, seed=3):
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.0, 4.0, (H, W, 4)).astype(np.float16)
    c[..., 3] = rng.uniform(0.0, 0.9, (H, W)).astype(np.float16)
    return c


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


@pytest.mark.parametrize("W,H", dof_inputs.SIZES)
def test_all_sky_is_a_bit_copy(W, H):
    g = dof_inputs.globals_set("defaults", W, H)
    color = _random_color(H, W)
    color[0, 0] = [np.nan, np.inf, -0.0, 65504.0]
    depth = np.ones((H, W), np.float32)
    depth[1, 1], depth[2, 2] = np.nan, 1.5            # not (depth < 1): copied too
    out, lq = dof_oracle.depth_of_field(g, depth, dof_oracle.chain(color))
    assert np.array_equal(_bits(out), _bits(color)) and (lq == -1).all()


@pytest.mark.parametrize("gname", dof_inputs.GLOBALS)
@pytest.mark.parametrize("W,H", dof_inputs.SIZES)
def test_constant_colour_at_every_lod(W, H, gname):
    """Power-of-two components: every product with a weight k/256 and every sum is exact, whatever the level."""
    g = dof_inputs.globals_set(gname, W, H)
    _, depth = dof_inputs.images(W, H)
    color = np.empty((H, W, 4), np.float16)
    color[:] = [0.5, 2.0, 0.125, 0.25]
    levels = dof_oracle.chain(color)
    for lv in levels:
        assert (lv == color[0, 0]).all()
    out, lq = dof_oracle.depth_of_field(g, depth, levels)
    geom = depth < 1.0
    assert set((lq[geom] >> 8).tolist()) == set(range(len(levels)))          # every level is selected
    assert (out[geom] == np.array([0.5, 2.0, 0.125, 1.0], np.float16)).all()
    assert (out[~geom] == color[0, 0]).all()


@pytest.mark.parametrize("gname", dof_inputs.GLOBALS)
def test_in_focus_pixels_average_their_wrapped_neighbours(gname):
    """Depth at plane_in_focus: c = 0 (to rounding), lod 0; the taps at uv +- one texel are the four neighbours, wrapped
    around the edges (REPEAT), summed in the shader's order."""
    W, H = 33, 17
    g = dof_inputs.globals_set(gname, W, H)
    color = _random_color(H, W)
    depth = np.full((H, W), dof_inputs.depth_from_distance(g, float(g.plane_in_focus)), np.float32)
    out, lq = dof_oracle.depth_of_field(g, depth, dof_oracle.chain(color))
    assert (lq == 0).all()
    c = color[..., :3].astype(np.float32)
    q = np.float32(0.25)
    want = ((np.roll(c, -1, 1) * q + np.roll(c, 1, 1) * q) + np.roll(c, -1, 0) * q) + np.roll(c, 1, 0) * q
    assert np.array_equal(_bits(out[..., :3]), _bits(want.astype(np.float16)))
    assert (out[..., 3] == 1.0).all()
    # the wrap: the left column's second tap is the right column
    x0 = ((c[:, 1] * q + c[:, W - 1] * q) + np.roll(c, -1, 0)[:, 0] * q) + np.roll(c, 1, 0)[:, 0] * q
    assert np.array_equal(_bits(out[:, 0, :3]), _bits(x0.astype(np.float16)))


@pytest.mark.parametrize("W,H", dof_inputs.SIZES)
def test_far_plane_pixels_are_the_top_level(W, H):
    """od = far: c = 1, rho = the frame's diagonal, past the last level (max_lod = L does not limit it): the clamp to
    level L - 1, whose one texel every tap returns."""
    g = dof_inputs.globals_set("defaults", W, H)
    color = _random_color(H, W)
    levels = dof_oracle.chain(color)
    depth = np.full((H, W), np.nextafter(np.float32(1.0), np.float32(0.0)), np.float32)   # the last depth below 1
    out, lq = dof_oracle.depth_of_field(g, depth, levels)
    assert levels[-1].shape == (1, 1, 4) and (lq == (len(levels) - 1) * 256).all()
    assert (out[..., :3] == levels[-1][0, 0, :3]).all() and (out[..., 3] == 1.0).all()


def test_chain_even_extents_are_2x2_means():
    color = _random_color(32, 64)
    levels = dof_oracle.chain(color)
    assert [lv.shape[:2] for lv in levels] == [(32, 64), (16, 32), (8, 16), (4, 8), (2, 4), (1, 2), (1, 1)]
    assert np.array_equal(_bits(levels[0]), _bits(color))
    h = np.float32(0.5)
    for k in range(1, 6):
        s = levels[k - 1].astype(np.float32)
        a, b, c, d = s[0::2, 0::2], s[0::2, 1::2], s[1::2, 0::2], s[1::2, 1::2]
        want = (a * h + b * h) * h + (c * h + d * h) * h
        assert np.array_equal(_bits(levels[k]), _bits(want.astype(np.float16))), k


def _exact_axis(n_dst, n_src):
    """blit_axis in exact rational arithmetic: [(i0, i1, weight numerator of i1 over 256)]."""
    out = []
    for x in range(n_dst):
        t = Fraction((2 * x + 1) * n_src, 2 * n_dst) - Fraction(1, 2)
        fx = (t * 256 + Fraction(1, 2)).__floor__()
        i, w = fx >> 8, fx & 255
        if i < 0:
            i, w = 0, 0
        elif i >= n_src - 1:
            i, w = n_src - 2, 256
        if n_src == 1:
            i, w = 0, 0
        out.append((i, min(i + 1, n_src - 1), w))
    return out


def test_chain_odd_extents():
    """97 -> 48 and 55 -> 27: the taps and 8-bit weights from exact rationals (no position is within rounding of a weight
    boundary: (2x + 1) n_src 128 / n_dst + 1/2 is never an integer for these extents), the texels from float64."""
    color = _random_color(55, 97)
    lv1 = dof_oracle.blit(color)
    assert lv1.shape == (27, 48, 4)
    ax, ay = _exact_axis(48, 97), _exact_axis(27, 55)
    x0, x1, wx = dof_oracle._blit_axis(48, 97, np.float32)
    y0, y1, wy = dof_oracle._blit_axis(27, 55, np.float32)
    assert [(int(a), int(b), int(w * 256)) for a, b, w in zip(x0, x1, wx)] == ax
    assert [(int(a), int(b), int(w * 256)) for a, b, w in zip(y0, y1, wy)] == ay
    assert any(w not in (0, 128, 256) for _, _, w in ax)
    s = color.astype(np.float64)
    want = np.empty((27, 48, 4))
    for y, (j0, j1, wj) in enumerate(ay):
        for x, (i0, i1, wi) in enumerate(ax):
            fx, fy = wi / 256.0, wj / 256.0
            want[y, x] = (s[j0, i0] * (1 - fx) + s[j0, i1] * fx) * (1 - fy) + (s[j1, i0] * (1 - fx) + s[j1, i1] * fx) * fy
    # the float32 filter is within an fp32 rounding of the float64 one: the same float16, or its neighbour at a tie
    assert helpers.f16_close(lv1, want.astype(np.float16)).all()
    assert (lv1 == want.astype(np.float16)).mean() > 0.99


def test_chain_degenerate_5x3():
    """5x3 -> 2x1 -> 1x1 by hand: 5 -> 2 taps (0, 1; 3/4) and (3, 4; 1/4); 3 -> 1 samples row 1 with weight 0 for row 2;
    2 -> 1 is the mean; an extent of 1 stays 1. Integer texels: every product and sum is exact."""
    color = np.arange(5 * 3 * 4, dtype=np.float32).reshape(3, 5, 4).astype(np.float16)
    levels = dof_oracle.chain(color)
    assert [lv.shape[:2] for lv in levels] == [(3, 5), (1, 2), (1, 1)]
    r = color[1].astype(np.float32)
    l1 = np.stack([r[0] * 0.25 + r[1] * 0.75, r[3] * 0.75 + r[4] * 0.25])[None]
    assert np.array_equal(levels[1].astype(np.float32), l1)
    assert np.array_equal(levels[2].astype(np.float32), (l1[:, 0] * 0.5 + l1[:, 1] * 0.5)[None])


@pytest.mark.parametrize("gname", dof_inputs.GLOBALS)
@pytest.mark.parametrize("W,H", dof_inputs.SIZES)
def test_float64_moves_lq_by_at_most_one_step(W, H, gname):
    _, lq32 = dof_inputs.reference(W, H, gname, np.float32)
    _, lq64 = dof_inputs.reference(W, H, gname, np.float64)
    geom = lq32 >= 0
    assert (geom == (lq64 >= 0)).all()
    L = dof_oracle.level_count(W, H)
    assert set((lq32[geom] >> 8).tolist()) == set(range(L))                  # the inputs select every level
    share0 = float((lq32[geom] == 0).mean())
    assert 0.10 <= share0 <= 0.66, share0
    moved = (lq32 != lq64)[geom]
    print(f"dof lq float64 vs float32 {W}x{H} {gname}: {moved.mean():.4%} of {int(geom.sum())} geometry pixels")
    assert np.abs(lq32 - lq64).max() <= 1
    assert moved.mean() <= F64_CAP


def test_lq_offset_moves_only_geometry_pixels():
    W, H = 64, 36
    base, lq = dof_inputs.reference(W, H, "focus20")
    for off in (-1, 1):
        other, lqo = dof_inputs.reference(W, H, "focus20", np.float32, off)
        geom = lq >= 0
        assert np.array_equal(_bits(other[~geom]), _bits(base[~geom]))
        assert (np.abs(lqo[geom] - lq[geom]) <= 1).all() and (lqo[geom] != lq[geom]).any()
        assert (_bits(other) != _bits(base)).any()
