"""Parity of every HIP pass against the CPU oracle at non-default renderer settings (-m gpu).

tests/test_gpu_parity.py runs every pass at soc.globals_defaults(); the reference exposes the settings below as live
editor properties (renderer.cpp:690-770) and the kernels choose their code by them. Each test here is one pass,
parametrised over the named variants of helpers.SETTINGS_VARIANTS that the pass reads (the C oracle is cross-checked
with the float64 restatement at the same variants in test_oracle_settings.py), at 200 x 120 (even width, 16-B rows,
W % 8 == 0, a partial tile at the right and bottom of the SSAO 64 x 16, composition 32 x 16 and TAA 128 x 4 tiles) and
97 x 55 (every pair path falls back).

Bounds (test_gpu_parity.py's docstring): RGBA16F outputs |d| <= 1e-3 + 2e-3|ref| on every value; SSAO R8
within 2 levels on >= 99.5 % of the pixels, mean <= 0.5, max <= 2 + SSAO_FLIPS * 255 / ssao_kernel_size; histogram
bit-exact; exposure within 1e-5; tone-mapped RGBA8 within 1 level on >= 99.9 % and 2 anywhere, RGBA32F within 2e-3;
clouds RGBA8 within 2 levels on >= 99.5 % (test_clouds).

The launch each SSAO case reaches is named in its id, read from soc_ssao_generation's dispatch (ssao.hip).
"""
import numpy as np
import pytest
import torch

import np_oracle as npo
from helpers import (SSAO_FLIPS, apply_variant, boundary_colours, cached_variant_inputs, f16_close, frame_parity,
                     globals_for, host_frame, random_rgba16, set_lights, smooth_rgba16, sponza_inputs, variants_for)

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(200, 120), (97, 55)]
SHAPE_IDS = ["200x120", "97x55"]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def inputs(name, W, H, **kw):
    return cached_variant_inputs(name, W, H, shadow_size=256, **kw)


def copy_globals(g):
    return type(g).from_buffer_copy(bytes(g))


# ------------------------------------------------------------------------------------------------ SSAO
# (variant, noise table, tuning knobs, the launch of ssao.hip's dispatch). sip: the inverse projection is sparse with a
# positive w row; full: min(ssao_kernel_size, 26) == 26; persp: the projection's w row is (0, 0, -1, 0). The seven
# launches: ssao_pipe_kernel<persp> / <affine> (table, sip, full, tiled), ssao_kernel<table,sip,full> (SOC_SSAO_TILE=0),
# <table,sip,partial>, <table,general> (any kernel size), <hash,sip,full>, <hash,general> (not sip, or not full).
SSAO_CASES = [
    ("default", True, {}, "ssao_pipe_kernel<persp>"),
    ("ssao_k40", True, {}, "ssao_pipe_kernel<persp>"),           # 26 taps, divisor 40
    ("ssao_r005", True, {}, "ssao_pipe_kernel<persp>"),
    ("ssao_r1", True, {}, "ssao_pipe_kernel<persp>"),
    ("ssao_bias0", True, {}, "ssao_pipe_kernel<persp>"),
    ("ssao_bias01", True, {}, "ssao_pipe_kernel<persp>"),
    ("ssao_ortho", True, {}, "ssao_pipe_kernel<affine>"),
    ("ssao_r1", True, {"SOC_SSAO_TILE": "0"}, "ssao_kernel<table,sip,full>"),
    ("ssao_ortho", True, {"SOC_SSAO_TILE": "0"}, "ssao_kernel<table,sip,full>"),
    ("ssao_k1", True, {}, "ssao_kernel<table,sip,partial>"),
    ("ssao_k8", True, {}, "ssao_kernel<table,sip,partial>"),
    ("ssao_k25", True, {}, "ssao_kernel<table,sip,partial>"),
    ("ssao_k8_r1_bias0", True, {}, "ssao_kernel<table,sip,partial>"),
    ("ssao_ortho_k8", True, {}, "ssao_kernel<table,sip,partial>"),
    ("ssao_oblique", True, {}, "ssao_kernel<table,general>"),
    ("ssao_oblique_r1_bias01", True, {}, "ssao_kernel<table,general>"),
    ("default", False, {}, "ssao_kernel<hash,sip,full>"),
    ("ssao_k40", False, {}, "ssao_kernel<hash,sip,full>"),
    ("ssao_bias0", False, {}, "ssao_kernel<hash,sip,full>"),
    ("ssao_ortho", False, {}, "ssao_kernel<hash,sip,full>"),
    ("ssao_k8", False, {}, "ssao_kernel<hash,general>"),
    ("ssao_r005", False, {}, "ssao_kernel<hash,sip,full>"),
    ("ssao_oblique", False, {}, "ssao_kernel<hash,general>"),
]


def _ssao_id(c):
    return f"{c[0]}-{'table' if c[1] else 'hash'}{'-tile0' if c[2] else ''}[{c[3]}]"


@pytest.mark.parametrize("W,H", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("case", SSAO_CASES, ids=_ssao_id)
def test_ssao_generation(soc, oracle, monkeypatch, case, W, H):
    """soc.ssao_generation against oracle.ssao_generation at kernel sizes 1 / 8 / 25 / 40, radii 0.05 / 1, biases 0 /
    0.1, with the noise table and with the in-kernel hash, through the reference's perspective, an orthographic camera
    (sparse inverse, not persp: on a height field) and an oblique near plane (inverse not sparse), each with its true
    inverse. The oracle's AO image must be finite by construction (R8) and not constant (std > 5 levels)."""
    name, with_table, knobs, _launch = case
    g, gb = inputs(name, W, H)
    ksize = int(g.ssao_kernel_size)
    ref = np.zeros((H // 2, W // 2), np.uint8)
    oracle.ssao_generation(g, gb["depth"], gb["normal"], ref)
    assert ref.astype(np.float64).std() > 5.0, ref.astype(np.float64).std()      # the AO image is not constant
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    soc.reload_tuning()
    depth, normal = dev(gb["depth"]), dev(gb["normal"])
    out = torch.zeros(H // 2, W // 2, dtype=torch.uint8, device=DEV)
    table = None
    if with_table:
        table = torch.zeros((H // 2) * (W // 2) * 2, dtype=torch.float32, device=DEV)
        soc.ssao_prepare_noise(normal, out, table)
    soc.ssao_generation(g, depth, normal, out, table)
    d = np.abs(host(out).astype(np.int32) - ref.astype(np.int32))
    print(f"ssao {_ssao_id(case)} {W}x{H}: within2 {(d <= 2).mean():.5f} mean {d.mean():.4f} max {d.max()}")
    assert (d <= 2).mean() >= 0.995, (d.max(), (d <= 2).mean())
    assert d.mean() <= 0.5, d.mean()
    assert d.max() <= 2 + SSAO_FLIPS * 255.0 / ksize, d.max()


# ------------------------------------------------------------------------------------------------ composition
def _half_tolerance_mask(a, ref):
    """Pixels with a channel where |a - ref| > (1e-3 + 2e-3 |ref|) / 2 (or a NaN on one side only)."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore"):
        over = ~(np.abs(a - ref) <= 0.5 * (1e-3 + 2e-3 * np.abs(ref)))
    over &= ~(np.isnan(a) & np.isnan(ref))
    return over.any(axis=-1)


@pytest.mark.parametrize("W,H", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("lights", [0, 3], ids=["nolights", "1point2spot"])
@pytest.mark.parametrize("name", variants_for("composition"))
def test_composition(soc, oracle, name, lights, W, H):
    """soc.composition against the oracle; soc.composition_luminance_histogram gives the same colour bits and the
    oracle's bins of that colour, at the variant's log range and at the narrow one (-2, 2). Pixels where the fp32 oracle
    itself is more than half the tolerance from the float64 restatement (an ill-conditioned input: the ESM exponent at
    exponential_factor -200) are left out, at most 1 % of them; the share is printed."""
    g, gb = inputs(name, W, H)
    if lights:
        set_lights(g, 1, 2)
    rng = np.random.default_rng(W + lights)
    ssao = rng.integers(0, 256, (H // 2, W // 2), dtype=np.uint8)      # the full range, zeros included
    ssao[rng.uniform(size=ssao.shape) < 0.05] = 0
    clouds = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    ref = np.zeros((H, W, 4), np.float16)
    oracle.composition(g, ref, gb["albedo"], gb["emissive"], gb["normal"], gb["depth"], ssao, gb["shadow"], clouds)
    old, npo.SUBTEXEL_BITS = npo.SUBTEXEL_BITS, 8
    try:
        ref64 = npo.composition(g, gb["albedo"], gb["emissive"], gb["normal"], gb["depth"], ssao, gb["shadow"], clouds)
    finally:
        npo.SUBTEXEL_BITS = old
    ill = _half_tolerance_mask(ref, ref64)
    print(f"composition {name} lights={lights} {W}x{H}: {ill.mean():.4%} of the pixels left out (oracle beyond half the "
          f"tolerance of float64)")
    assert ill.mean() <= 0.01, ill.mean()
    dg = soc.globals_device_buffer()
    soc.upload_globals(g, dg)
    ins = [dev(gb[k]) for k in ("albedo", "emissive", "normal", "depth")]
    d_ssao, d_shadow, d_clouds = dev(ssao), dev(gb["shadow"]), dev(clouds)
    out = torch.zeros(H, W, 4, dtype=torch.float16, device=DEV)
    soc.composition(g, out, *ins, d_ssao, d_shadow, d_clouds, d_globals=dg)
    got = host(out)
    ok = f16_close(got, ref) | ill[..., None]
    assert ok.all(), (ok.mean(), np.argwhere(~ok)[:5], got[~ok][:5], ref[~ok][:5])
    sky = gb["depth"] == 1.0
    assert np.array_equal(got[sky].view(np.uint16), ref[sky].view(np.uint16))   # sky = the clouds texel, exact
    for log_range in (None, "log_narrow"):
        gh = copy_globals(g)
        if log_range:
            apply_variant(gh, log_range)
            soc.upload_globals(gh, dg)
        out2 = torch.zeros(H, W, 4, dtype=torch.float16, device=DEV)
        ae = soc.auto_exposure_buffer()
        soc.composition_luminance_histogram(gh, out2, *ins, d_ssao, d_shadow, d_clouds, ae, soc.histogram_scratch(),
                                            d_globals=dg)
        got2 = host(out2)
        assert np.array_equal(got2.view(np.uint16), got.view(np.uint16))
        ae_ref = soc.AutoExposure()
        oracle.generate_luminance_histogram(gh, got2, ae_ref)
        assert np.array_equal(host(ae)[1:].astype(np.int64), np.array(ae_ref.histogram_buckets, np.int64)), log_range


# ------------------------------------------------------------------------------------------------ tone mapping
def _special_rgba16(H, W, seed):
    """Random colours in [-0.5, 6) with 0, negatives, 65504 and +-inf planted (whole pixels and single channels)."""
    img = random_rgba16(H, W, seed=seed, lo=-0.5, hi=6.0)
    rng = np.random.default_rng(seed + 1)
    specials = [0.0, -1.0, -65504.0, 65504.0, np.inf, -np.inf]
    for i, v in enumerate(specials):
        n = 2 if np.isinf(v) else 6
        ys, xs = rng.integers(0, H, 2 * n), rng.integers(0, W, 2 * n)
        img[ys[:n], xs[:n], :3] = np.float16(v)                      # the whole pixel
        img[ys[n:], xs[n:], i % 3] = np.float16(v)                   # one channel
    ys, xs = rng.integers(0, H, 2), rng.integers(0, W, 2)
    img[ys, xs, 0], img[ys, xs, 1] = np.float16(np.inf), np.float16(-np.inf)
    return img


@pytest.mark.parametrize("W,H", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("fmt", ["RGBA8_UNORM", "RGBA32F", "RGBA8_SRGB"])
@pytest.mark.parametrize("name", variants_for("tonemap"))
def test_tone_mapping(soc, oracle, name, fmt, W, H):
    """Inputs with 0, negatives, 65504 and +-inf. The C oracle reads the colour through its bilinear sampler
    (tone_mapping.inl's texture() at the pixel centre): the neighbour's weight is 0 and 0 x inf is NaN, so the pixels left
    of and above an infinite texel come out black there, while the kernel fetches the texel (as the float64 restatement
    does). Those pixels, where the fp32 oracle is beyond half the RGBA32F tolerance of the float64 restatement, are left
    out: at most 1 % of them; the share is printed."""
    g = apply_variant(globals_for(W, H), name)
    img = _special_rgba16(H, W, seed=4)
    F = getattr(soc, "FMT_" + fmt)
    for exposure in (-3.0, 1.5):
        ae = soc.AutoExposure()
        ae.exposure = exposure
        ref32 = np.zeros((H, W, 4), np.float32)
        oracle.tone_mapping(g, img, ae, ref32, soc.FMT_RGBA32F)
        with np.errstate(invalid="ignore"):
            ill = ~(np.abs(ref32 - npo.tone_mapping(g, img, exposure, raw=True)) <= 1e-3).all(axis=-1)
        print(f"tone map {name} {fmt} {W}x{H} exposure {exposure}: {ill.mean():.4%} of the pixels left out")
        assert ill.mean() <= 0.01, ill.mean()
        if fmt == "RGBA32F":
            ref = np.zeros((H, W, 4), np.float32)
            out = torch.zeros(H, W, 4, dtype=torch.float32, device=DEV)
        else:
            ref = np.zeros((H, W, 4), np.uint8)
            out = torch.zeros(H, W, 4, dtype=torch.uint8, device=DEV)
        oracle.tone_mapping(g, img, ae, ref, F)
        soc.tone_mapping(g, dev(img), soc.auto_exposure_buffer(exposure=exposure), out, F)
        got = host(out)
        if fmt == "RGBA32F":
            assert np.isfinite(got).all()
            d = np.abs(got - ref)[~ill]
            assert d.max() <= 2e-3, (exposure, d.max())
        else:
            d = np.abs(got.astype(np.int32) - ref.astype(np.int32))[~ill]
            assert (d <= 1).mean() >= 0.999 and d.max() <= 2, (exposure, (d <= 1).mean(), d.max())


@pytest.mark.parametrize("W,H", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
@pytest.mark.parametrize("name", variants_for("tonemap"))
def test_taa_tone_mapping_fused_equals_two_passes(soc, name, srgb, W, H):
    """The fused TAA + tone-map launch gives the TAA pass's bits and the tone-map pass's codes at every tone-map
    variant and both exposures (97 x 55: the two-pass fallback), on inputs with 0, negatives, 65504 and +-inf."""
    fmt = soc.FMT_RGBA8_SRGB if srgb else None
    g, gb = inputs("default", W, H)
    apply_variant(g, name)
    cur, prev = dev(_special_rgba16(H, W, seed=1)), dev(_special_rgba16(H, W, seed=2))
    pvel = gb["velocity"].copy()
    pvel[..., :2] += np.float16(0.0015)
    vel, pvel, depth = dev(gb["velocity"]), dev(pvel), dev(gb["depth"])
    for exposure in (-3.0, 1.5):
        ae = soc.auto_exposure_buffer(exposure=exposure)
        t1 = torch.zeros(H, W, 4, dtype=torch.float16, device=DEV)
        o1 = torch.zeros(H, W, 4, dtype=torch.uint8, device=DEV)
        soc.temporal_antialiasing(g, t1, cur, prev, vel, pvel, depth)
        soc.tone_mapping(g, t1, ae, o1, target_format=fmt)
        t2, o2, v2 = torch.zeros_like(t1), torch.zeros_like(o1), torch.zeros_like(t1)
        soc.temporal_antialiasing_tone_mapping(g, t2, cur, prev, vel, pvel, depth, ae, o2, velocity_history_out=v2,
                                               output_format=fmt)
        torch.cuda.synchronize()
        assert torch.equal(t1.view(torch.int16), t2.view(torch.int16))      # bits: NaN (inf - inf) included
        assert torch.equal(v2, vel)
        d = (o1.int() - o2.int()).abs()
        assert int(d.max()) <= 1 and float((d > 0).float().mean()) < 1e-4, (exposure, int(d.max()))


# ------------------------------------------------------------------------------------------------ auto exposure
@pytest.mark.parametrize("W,H", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("name", ["default", "log_narrow", "log_wide", "res_clip", "all_at_once"])
def test_histogram_bit_exact(soc, oracle, name, W, H):
    """Half the pixels within 1e-3 of a bin boundary of the variant's log range (the fast bin's exact fallback), +-inf
    pixels, +inf and -inf in one pixel (a NaN luminance), NaN and black pixels; res_clip: resolution smaller than the
    image (only the top-left resolution[0] x resolution[1] pixels are binned)."""
    g = apply_variant(globals_for(W, H), name)
    rng = np.random.default_rng(H)
    img = np.exp(rng.normal(-1.0, 3.0, (H, W, 4))).astype(np.float16)
    sel = rng.uniform(size=(H, W)) < 0.5
    img[sel] = boundary_colours(g, int(sel.sum()), rng)
    img[rng.uniform(size=(H, W)) < 0.03] = 0.0
    for k, rgb in enumerate([(np.inf, np.inf, np.inf), (-np.inf, -np.inf, -np.inf), (np.inf, -np.inf, 1.0),
                             (1.0, np.inf, -np.inf), (-np.inf, 2.0, np.inf), (np.inf, 0.5, 0.5), (0.5, -np.inf, 0.5),
                             (np.nan, 1.0, 1.0)]):
        ys, xs = rng.integers(0, H, 9), rng.integers(0, W, 9)
        img[ys, xs, :3] = np.array(rgb, np.float16)
    ae = soc.AutoExposure()
    oracle.generate_luminance_histogram(g, img, ae)
    ref = np.array(ae.histogram_buckets, np.int64)
    buf = soc.auto_exposure_buffer()
    soc.generate_luminance_histogram(g, dev(img), buf)
    got = host(buf)[1:].astype(np.int64)
    assert got.sum() == min(W, int(g.resolution[0])) * min(H, int(g.resolution[1]))
    assert np.array_equal(got, ref), np.nonzero(got != ref)


def _bins(kind, pixels):
    bins = np.zeros(256, np.uint32)
    if kind == "bin0":
        bins[0] = pixels
    elif kind == "bin255":
        bins[255] = pixels
    elif kind == "middle":
        bins[117] = pixels
    else:
        bins[250] = pixels
    return bins


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("kind", ["bin0", "bin255", "middle", "20M_in_bin250"])
@pytest.mark.parametrize("name", variants_for("exposure"))
def test_resolve(soc, oracle, name, kind, wide):
    """Hand-written bins: an all-black frame (the max(..., 1) denominator), every pixel in the last bin, one middle bin,
    and 20 000 000 pixels in bin 250 with total_pixels set (the narrow u32 tree wraps at 5e9 mod 2^32, as the oracle
    models; the wide sum exceeds 2^32), at delta_time x adjustment_speed 0 (alpha 0) and 1e3 (alpha clamps to 1),
    target luminances 0.05 and 1.0 and the narrow and wide log ranges."""
    W, H = 640, 360
    g = apply_variant(globals_for(W, H), name)
    g.resolution[0], g.resolution[1] = W, H
    big = kind == "20M_in_bin250"
    pixels = 20_000_000 if big else W * H
    bins = _bins(kind, pixels)
    ae = soc.AutoExposure()
    ae.exposure = 0.37
    ae.histogram_buckets[:] = [int(b) for b in bins]
    oracle.resolve_luminance_histogram(g, ae, pixels if big else 0, wide)
    assert np.isfinite(ae.exposure)
    buf = soc.auto_exposure_buffer(exposure=0.37)
    buf[1:] = torch.from_numpy(bins.view(np.int32)).to(DEV)
    soc.resolve_luminance_histogram(g, buf, pixels if big else 0, wide)
    assert abs(soc.exposure_of(buf) - ae.exposure) <= 1e-5, (soc.exposure_of(buf), ae.exposure)
    assert int(host(buf)[1:].sum()) == 0


# ------------------------------------------------------------------------------------------------ TAA
# (id, variant, extent, depth, history, velocity)
TAA_CASES = [
    ("fc0-200x120[taa_lds]", "fc0", (200, 120), "scene", "noise", "scene"),
    ("fc0-97x55[taa_fast]", "fc0", (97, 55), "scene", "noise", "scene"),
    ("fc1-200x120[taa_lds]", "fc1", (200, 120), "scene", "noise", "scene"),
    ("fc1-97x55[taa_fast]", "fc1", (97, 55), "scene", "noise", "scene"),
    ("default-offscreen-200x120[taa_lds]", "default", (200, 120), "scene", "noise", "offscreen"),
    ("default-offscreen-97x55[taa_fast]", "default", (97, 55), "scene", "noise", "offscreen"),
    ("default-allsky-200x120[taa_lds]", "default", (200, 120), "allsky", "noise", "scene"),
    ("fc0-allsky-97x55[taa_fast]", "fc0", (97, 55), "allsky", "noise", "scene"),
    ("res2x-96x54-random_depth[taa_generic]", "res2x", (96, 54), "random", "noise", "scene"),
    ("res2x-96x54-allsky[taa_generic]", "res2x", (96, 54), "allsky", "noise", "offscreen"),
    ("res2x-96x54-scene-smooth_history[taa_generic]", "res2x", (96, 54), "scene", "smooth", "scene"),
    ("res2x-fc0-97x55-random_depth[taa_generic]", "res2x+fc0", (97, 55), "random", "noise", "scene"),
]


@pytest.mark.parametrize("case", TAA_CASES, ids=lambda c: c[0])
def test_taa(soc, oracle, case):
    """Previous velocity = velocity + 0.036 in x and y: the disocclusion weight is ~0.5, so a wrong Gaussian weight of
    `blurred` moves the result by half its error. offscreen: the right 30 % of the frame reads its history half a
    frame to the right (accum 1). res2x: resolution (2W, 2H), the 3 x 3 taps half a texel apart (taa_generic with pox /
    poy from the globals); the scene's depth then only with a smooth history (test_oracle_settings.test_taa: the
    closest of near-tied interpolated depths depends on the rounding order)."""
    _id, name, (W, H), depth_kind, history, vel_kind = case
    g, gb = inputs("default", W, H)
    for n in name.split("+"):
        apply_variant(g, n)
    rng = np.random.default_rng(W)
    cur = random_rgba16(H, W, seed=1, hi=3.0)
    prev = random_rgba16(H, W, seed=2, hi=3.0) if history == "noise" else smooth_rgba16(H, W)
    depth = {"scene": gb["depth"], "random": rng.uniform(0.5, 0.9, (H, W)).astype(np.float32),
             "allsky": np.ones((H, W), np.float32)}[depth_kind]
    vel = gb["velocity"].copy()
    if vel_kind == "offscreen":
        vel[:, int(0.7 * W):, 0] = np.float16(-0.5)
    pvel = vel.copy()
    pvel[..., :2] += np.float16(0.036)
    if vel_kind == "offscreen":      # >= 25 % of the history taps leave the screen (measured on the oracle's own taps)
        u = (np.arange(W) + 0.5) / W
        assert ((u[None, :] - vel[..., 0].astype(np.float64)) > 1.0).mean() >= 0.25
    ref = np.zeros((H, W, 4), np.float16)
    oracle.temporal_antialiasing(g, ref, cur, prev, vel, pvel, depth)
    out = torch.zeros(H, W, 4, dtype=torch.float16, device=DEV)
    vout = torch.zeros(H, W, 4, dtype=torch.float16, device=DEV)
    soc.temporal_antialiasing(g, out, dev(cur), dev(prev), dev(vel), dev(pvel), dev(depth), vout)
    ok = f16_close(host(out), ref)
    assert ok.all(), (ok.mean(), np.argwhere(~ok)[:5])
    assert np.array_equal(host(vout).view(np.uint16), vel.view(np.uint16))


# ------------------------------------------------------------------------------------------------ clouds
@pytest.mark.parametrize("compact", [False, True], ids=["single_lane", "workspace"])
@pytest.mark.parametrize("cam_y", [2.2, 900.0])
@pytest.mark.parametrize("name", ["sun_el3", "sun_el35", "sun_el80", "t0", "t1234"])
def test_clouds(soc, oracle, name, cam_y, compact):
    W, H = 160, 90
    g, gb = inputs(name, W, H, camera=((-14.0, cam_y, 0.3), (0.0, -0.42, 0.0)), elapsed=10.0)
    if cam_y > 100.0:
        gb["depth"][...] = 1.0      # above the atrium: all sky
    assert (gb["depth"] == 1.0).mean() > 0.05
    ref = np.zeros((H, W, 4), np.uint8)
    oracle.cloud_rendering(g, gb["depth"], gb["noise"], ref)
    out = torch.zeros(H, W, 4, dtype=torch.uint8, device=DEV)
    ws = soc.cloud_rendering_workspace(W, H) if compact else None
    soc.cloud_rendering(g, dev(gb["depth"]), dev(gb["noise"]), out, ws)
    d = np.abs(host(out).astype(np.int32) - ref.astype(np.int32))
    print(f"clouds {name} cam_y={cam_y} compact={compact}: within2 {(d <= 2).mean():.5f} max {d.max()}")
    assert (d <= 2).mean() >= 0.995, ((d <= 2).mean(), d.max())
    nonsky = gb["depth"] < 1.0
    assert (host(out)[nonsky][:, :3] == np.array([51, 102, 255], np.uint8)).all()


# ------------------------------------------------------------------------------------------------ render graph
def test_render_graph_settings_change_between_frames(soc, oracle):
    """soc.Renderer, three frames: defaults, then the SSAO, composition, exposure and tone-map settings all changed at
    once, then the defaults again. A parameter cached at creation, or left in the device globals, shows up in the second
    or third frame's parity."""
    W, H = 256, 144
    g0, gb = sponza_inputs(W, H, elapsed=10.0)
    g1 = apply_variant(copy_globals(g0), "all_at_once")
    fr = soc.alloc_frame(W, H, DEV)
    for k in ("albedo", "emissive", "normal", "velocity", "depth"):
        fr[k].copy_(torch.from_numpy(gb[k]))
    fr["shadow"] = dev(gb["shadow"])
    fr["noise"].copy_(torch.from_numpy(gb["noise"]))
    r = soc.Renderer(fr)
    hf = host_frame(W, H, gb)
    ae = soc.AutoExposure()
    hist = 0
    for f, g in enumerate((g0, g1, g0)):
        fr["emissive"].copy_(dev(gb["emissive"]))           # bloom overwrites emissive each frame (quirk Q5)
        hf["emissive"][...] = gb["emissive"]
        e0 = soc.exposure_of(fr["auto_exposure"])
        r.execute(g)
        hist = oracle.frame(g, hf, ae, hist=hist)
        torch.cuda.synchronize()
        assert r.current_history() == hist
        frame_parity(soc, oracle, g, fr, hf, ae, hist, f"settings {W}x{H} frame {f}", e0,
                     ssao_step=255.0 / int(g.ssao_kernel_size))
    r.close()
