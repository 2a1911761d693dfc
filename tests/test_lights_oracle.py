"""tests/lights_oracle.py, the numpy restatement of Composition with bounded lights, against oracle/np_oracle.py and
against its own stated semantics (no GPU)."""
import numpy as np
import pytest

import light_bounds_scene as scene
import lights_oracle as lo
import np_oracle as npo

W, H = 64, 36


@pytest.fixture(scope="module")
def frame(soc):
    g, gb, ssao, clouds = scene.frame_inputs(W, H)
    return g, (gb["albedo"], gb["emissive"], gb["normal"], gb["depth"], ssao, gb["shadow"], clouds)


def bits(a):
    return np.asarray(a).view(np.uint16)


def test_unlimited_point_lights_are_np_oracle_bit_for_bit(frame):
    g, ins = frame
    g.spot_light_count = 0
    try:
        out, reach, lit = lo.composition(g, *ins, [0.0] * 6, [])
        ref = npo.composition(g, *ins)
    finally:
        scene.set_lights(g)
    assert np.array_equal(bits(out), bits(ref))
    assert reach.shape == (5, 4, 6) and (reach == lit[..., None]).all()


def test_unlimited_spot_lights_equal_np_oracle_where_it_is_a_number(frame):
    """The select drops a spot light outside its cone, where np_oracle adds its term times zero: the same value unless
    that term is NaN or Inf."""
    g, ins = frame
    out, _, _ = lo.composition(g, *ins, [0.0] * 6, [0.0] * 6)
    ref = npo.composition(g, *ins)
    ok = ~np.isnan(ref.astype(np.float32))
    assert ok.mean() > 0.99
    assert np.array_equal(bits(out)[ok], bits(ref)[ok])


def test_window_values():
    """w = clamp(1 - (d^2 / r^2)^2, 0, 1): 15/16 at d = r / 2, 0 from d = r on, 1 at the light."""
    for dt in (np.float64, np.float32):
        assert lo.window(dt(1.0), 2.0, dt) == dt(0.9375)
        assert lo.window(dt(4.0), 2.0, dt) == 0 and lo.window(dt(9.0), 2.0, dt) == 0 and lo.window(dt(0.0), 2.0, dt) == 1


def _one_point_light(g, world_point, offset, rng_range):
    g.point_light_count, g.spot_light_count = 1, 0
    L = g.point_lights[0]
    L.position[:] = [float(world_point[0] + offset[0]), float(world_point[1] + offset[1]), float(world_point[2] + offset[2])]
    L.color[:] = [1.0, 0.5, 0.25]
    L.intensity = 2.0
    return rng_range


def test_half_range_scales_the_term_by_15_16(frame):
    """A light at exactly d = r / 2 from a pixel (offsets and range exact in binary): the pixel's light term, recovered as
    the difference to the frame without lights before the RGBA16F rounding, is 0.9375 of the unbounded term."""
    g, ins = frame
    albedo, emissive, normal, depth = ins[:4]
    y, x = np.argwhere(depth != 1.0)[len(np.argwhere(depth != 1.0)) // 2]
    # the pixel's world position as the oracle forms it
    u, v = npo.centres(W, H)
    clip = np.array([u[y, x] * 2 - 1, v[y, x] * 2 - 1, float(depth[y, x]), 1.0])
    vs = npo.mat(g.camera_inverse_projection_matrix) @ clip
    world = (npo.mat(g.camera_inverse_view_matrix) @ (vs / vs[3]))[:3]
    try:
        # the light sits at the pixel's world position + (0, 1, 0) after rounding to fp32: measure d as the oracle sees it
        _one_point_light(g, world, (0.0, 1.0, 0.0), None)
        lp = np.array(list(g.point_lights[0].position), np.float64)
        d = np.linalg.norm(lp - world)
        terms = {}
        for name, r in (("none", None), ("unlimited", 0.0), ("bounded", 2.0 * d)):
            g.point_light_count = 0 if r is None else 1
            terms[name] = _direct(g, ins, [] if r is None else [r], y, x)
    finally:
        scene.set_lights(g)
    unl, bnd = terms["unlimited"] - terms["none"], terms["bounded"] - terms["none"]
    assert (unl > 0).all()
    # d / r = 1/2 to within the rounding of 2 * d: (d^2 / r^2)^2 = 1/16 to ~1e-16
    np.testing.assert_allclose(bnd / unl, 0.9375, rtol=1e-12)


def _direct(g, ins, point_ranges, y, x):
    """The float64 colour of pixel (y, x) before the RGBA16F store."""
    return lo.composition(g, *ins, point_ranges, [], linear=True)[0][y, x].astype(np.float64)


def test_beyond_the_range_is_the_frame_without_the_light(frame):
    """Every pixel at d >= r of a ranged light has the bits of the frame rendered without that light (and some pixels
    are inside the range, so the comparison is not of two equal frames)."""
    g, ins = frame
    k = 2                                    # POINTS[2]: range 5, reaches part of the frame
    r = scene.POINT_RANGES[k]
    with_light, reach, _ = lo.composition(g, *ins, scene.POINT_RANGES, scene.SPOT_RANGES)
    assert reach[..., k].any() and not reach[..., k].all()
    # the same frame without light k
    pos = list(g.point_lights[k].position)
    keep = [i for i in range(6) if i != k]
    try:
        for j, i in enumerate(keep):
            src, dst = scene.POINTS[i], g.point_lights[j]
            dst.position[:], dst.color[:], dst.intensity = src[0], src[1], src[2]
        g.point_light_count = 5
        without, _, _ = lo.composition(g, *ins, [scene.POINT_RANGES[i] for i in keep], scene.SPOT_RANGES)
    finally:
        scene.set_lights(g)
    depth = ins[3]
    u, v = npo.centres(W, H)
    clip = np.stack([u * 2 - 1, v * 2 - 1, depth.astype(np.float64), np.ones((H, W))], -1)
    vs = npo.apply(npo.mat(g.camera_inverse_projection_matrix), clip)
    world = npo.apply(npo.mat(g.camera_inverse_view_matrix), vs / vs[..., 3:4])[..., :3]
    d = np.linalg.norm(np.array(pos) - world, axis=-1)
    outside = d >= r
    assert outside.any() and (~outside & (depth != 1.0)).any()
    assert np.array_equal(bits(with_light)[outside], bits(without)[outside])
    assert not np.array_equal(bits(with_light)[~outside], bits(without)[~outside])


def test_float32_form_is_within_the_store_tolerance(frame):
    from helpers import f16_close
    g, ins = frame
    a, ra, _ = lo.composition(g, *ins, scene.POINT_RANGES, scene.SPOT_RANGES)
    b, rb, _ = lo.composition(g, *ins, scene.POINT_RANGES, scene.SPOT_RANGES, dtype=np.float32)
    assert f16_close(b, a).all()
    assert (ra != rb).mean() < 0.02      # a patch whose only pixel in reach sits on the boundary may flip


def test_scene_is_not_vacuous(frame):
    g, ins = frame
    _, reach, lit = lo.composition(g, *ins, scene.POINT_RANGES, scene.SPOT_RANGES)
    per_light = reach[lit].sum(0)
    assert (per_light == 0).any() and (per_light == lit.sum()).any()
    assert 0.2 <= 1.0 - reach[lit].mean() <= 0.8
