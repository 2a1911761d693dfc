"""The two CPU restatements against each other at non-default renderer settings.

tests/test_np_oracle.py cross-checks oracle/soc_oracle.c (fp32, the checker of every GPU parity test) with
oracle/np_oracle.py (numpy, float64) at the renderer's defaults only. The GPU settings tests (test_gpu_settings.py)
compare the kernels with the C oracle at every named variant of helpers.SETTINGS_VARIANTS, so the C oracle is
cross-checked here at those same variants first, pass by pass (each numpy pass gets the C oracle's inputs), at 64 x 36
and 97 x 55, with the tolerances written at the top of test_np_oracle.py, unchanged.

Composition additionally reports the share of channels where the two restatements differ by more than half the RGBA16F
tolerance: the GPU test may leave exactly those pixels out (the fp32 oracle itself is ill-conditioned there, e.g. the
ESM exponent at exponential_factor -200), and that share must stay under 1 % for the oracle alone.
"""
import numpy as np
import pytest

import np_oracle as npo
from helpers import cached_variant_inputs, set_lights, smooth_rgba16, variants_for
from test_np_oracle import f16_ok, u8_diff

SIZES = [(64, 36), (97, 55)]
HALF_TOL_CAP = 0.01


@pytest.fixture(autouse=True)
def _subtexel8():
    old = npo.SUBTEXEL_BITS
    npo.SUBTEXEL_BITS = 8
    yield
    npo.SUBTEXEL_BITS = old


def inputs(name, W, H, **kw):
    return cached_variant_inputs(name, W, H, shadow_size=256, **kw)


def half_tol_share(a, ref):
    """Share of the pixels with a channel where |a - ref| > (1e-3 + 2e-3 |ref|) / 2."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore"):
        over = np.abs(a - ref) > 0.5 * (1e-3 + 2e-3 * np.abs(ref))
    return float(over.any(axis=-1).mean())


@pytest.mark.parametrize("W,H", SIZES, ids=["64x36", "97x55"])
@pytest.mark.parametrize("name", variants_for("ssao"))
def test_ssao_and_blur(name, W, H, soc, oracle):
    g, gb = inputs(name, W, H)
    ssao = np.zeros((H // 2, W // 2), np.uint8)
    oracle.ssao_generation(g, gb["depth"], gb["normal"], ssao)
    diff = u8_diff(npo.ssao_generation(g, gb["depth"], gb["normal"], (H // 2, W // 2)), ssao)
    # one tap flip moves a pixel by 255 / ssao_kernel_size levels (11 at the 26 of test_np_oracle's "max = one tap flip")
    flip = int(np.ceil(255.0 / g.ssao_kernel_size)) + 1
    assert (diff <= 2).mean() >= 0.99 and diff.max() <= max(11, flip), ((diff > 2).mean(), diff.max())
    blur = np.zeros_like(ssao)
    oracle.ssao_blur(g, ssao, blur)
    assert u8_diff(npo.ssao_blur(ssao), blur).max() <= 1


@pytest.mark.parametrize("W,H", SIZES, ids=["64x36", "97x55"])
@pytest.mark.parametrize("lights", [0, 3], ids=["nolights", "1point2spot"])
@pytest.mark.parametrize("name", variants_for("composition"))
def test_composition(name, lights, W, H, soc, oracle):
    g, gb = inputs(name, W, H)
    if lights:
        set_lights(g, 1, 2)
    rng = np.random.default_rng(W + lights)
    ssao = rng.integers(0, 256, (H // 2, W // 2), dtype=np.uint8)      # the full range, zeros included
    ssao[rng.uniform(size=ssao.shape) < 0.05] = 0
    clouds = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    color = np.zeros((H, W, 4), np.float16)
    oracle.composition(g, color, gb["albedo"], gb["emissive"], gb["normal"], gb["depth"], ssao, gb["shadow"], clouds)
    ref = npo.composition(g, gb["albedo"], gb["emissive"], gb["normal"], gb["depth"], ssao, gb["shadow"], clouds)
    share = half_tol_share(color, ref)
    print(f"composition {name} {W}x{H} lights={lights}: {share:.4%} of the pixels beyond half the tolerance")
    f16_ok(ref, color, frac=0.999 if lights else 1.0)
    assert share <= HALF_TOL_CAP, share


@pytest.mark.parametrize("W,H", SIZES, ids=["64x36", "97x55"])
@pytest.mark.parametrize("name", sorted(set(variants_for("exposure") + variants_for("tonemap"))))
def test_exposure_and_tone_map(name, W, H, soc, oracle):
    g, gb = inputs(name, W, H)
    rng = np.random.default_rng(H)
    color = np.exp(rng.normal(-1.0, 2.5, (H, W, 4))).astype(np.float16)
    color[rng.uniform(size=(H, W)) < 0.05] = 0.0
    color[..., 3] = 1.0
    ae = soc.AutoExposure()
    ae.exposure = 0.37
    oracle.generate_luminance_histogram(g, color, ae)
    ref_bins = np.array(ae.histogram_buckets, np.int64)
    # np_oracle bins the whole image; the reference dispatches over resolution (generate_luminance_histogram.inl:59-62)
    rw, rh = min(int(g.resolution[0]), W), min(int(g.resolution[1]), H)
    bins = npo.generate_luminance_histogram(g, color[:rh, :rw]).astype(np.int64)
    assert ref_bins.sum() == rw * rh
    assert np.abs(bins - ref_bins).sum() <= 2 * max(1, int(0.001 * W * H))
    oracle.resolve_luminance_histogram(g, ae)
    assert abs(npo.resolve_luminance_histogram(g, ref_bins, 0.37) - ae.exposure) <= 1e-5
    for exposure in (-3.0, 1.5):
        ae.exposure = exposure
        tm = np.zeros((H, W, 4), np.uint8)
        oracle.tone_mapping(g, color, ae, tm)
        assert u8_diff(npo.tone_mapping(g, color, exposure), tm).max() <= 1, exposure


@pytest.mark.parametrize("total,wide", [(20_000_000, False), (20_000_000, True)], ids=["narrow_wraps", "wide_above_2^32"])
def test_resolve_wrap(total, wide, soc, oracle):
    """20 000 000 pixels in bin 250: the narrow u32 tree wraps (resolve_luminance_histogram.inl:58-70, 5e9 mod 2^32),
    the wide sum does not."""
    g = soc.globals_defaults(64, 36)
    g.delta_time = 0.016
    ae = soc.AutoExposure()
    ae.exposure = 0.37
    bins = np.zeros(256, np.uint64)
    bins[250] = total
    ae.histogram_buckets[250] = total
    oracle.resolve_luminance_histogram(g, ae, total, wide)
    assert abs(npo.resolve_luminance_histogram(g, bins, 0.37, total, wide) - ae.exposure) <= 1e-5


@pytest.mark.parametrize("W,H", SIZES, ids=["64x36", "97x55"])
@pytest.mark.parametrize("depth_kind", ["scene", "random", "allsky"])
@pytest.mark.parametrize("name", variants_for("taa"))
def test_taa(name, depth_kind, W, H, soc, oracle):
    """Noise colour and history, previous velocity = velocity + 0.036 (disocclusion weight ~0.5: the Gaussian blur carries
    half the result). Where resolution is not the image extent the 3 x 3 depth taps fall between texels, neighbouring
    taps on a smooth surface interpolate to depths a few ulp apart, and which one is the closest (so where the velocity
    is read, :162-163, 173) is decided by the rounding order: float64 and fp32 pick different taps on 1-4 % of the
    pixels, and a noise history turns the moved tap into 0.02-0.06. There the scene's depth goes with a smooth history;
    the random depth (no near ties) and the all-sky one (exact ties only) keep the noise history."""
    g, gb = inputs(name, W, H)
    rng = np.random.default_rng(W)
    cur = rng.uniform(0.0, 3.0, (H, W, 4)).astype(np.float16)
    prev = cur[:, ::-1].copy()
    if depth_kind == "scene" and (int(g.resolution[0]), int(g.resolution[1])) != (W, H):
        prev = smooth_rgba16(H, W)
    depth = {"scene": gb["depth"], "random": rng.uniform(0.5, 0.9, (H, W)).astype(np.float32),
             "allsky": np.ones((H, W), np.float32)}[depth_kind]
    pvel = gb["velocity"].copy()
    pvel[..., :2] += np.float16(0.036)
    taa = np.zeros((H, W, 4), np.float16)
    oracle.temporal_antialiasing(g, taa, cur, prev, gb["velocity"], pvel, depth)
    f16_ok(npo.temporal_antialiasing(g, cur, prev, gb["velocity"], pvel, depth), taa, frac=0.999, max_abs=1e-2)


@pytest.mark.parametrize("W,H", SIZES, ids=["64x36", "97x55"])
@pytest.mark.parametrize("cam_y", [2.2, 900.0])
@pytest.mark.parametrize("name", variants_for("clouds"))
def test_clouds(name, cam_y, W, H, soc, oracle):
    g, gb = inputs(name, W, H, camera=((-14.0, cam_y, 0.3), (0.0, -0.42, 0.0)), elapsed=10.0)
    if cam_y > 100.0 or (gb["depth"] == 1.0).mean() < 0.05:
        gb["depth"][...] = 1.0      # above the atrium (or the height field, which has no sky): all sky
    clouds = np.zeros((H, W, 4), np.uint8)
    oracle.cloud_rendering(g, gb["depth"], gb["noise"], clouds)
    diff = u8_diff(npo.cloud_rendering(g, gb["depth"], gb["noise"]), clouds)
    assert (diff <= 2).mean() >= 0.99 and diff.max() <= 16, ((diff > 2).mean(), diff.max())
