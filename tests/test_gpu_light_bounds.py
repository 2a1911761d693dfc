"""Composition with bounded lights on the GPU (soc_composition_bounded, soc_composition_luminance_histogram_bounded,
soc_renderer_set_light_bounds) against tests/lights_oracle.py.

Extents: 64x36 (the pair path with a partial last tile row), 98x56 (partial tiles on both axes) and 97x55 (odd width:
composition_generic, every pixel by its own test, no wave patches). The lights are light_bounds_scene's six point and six
spot lights with mixed ranges; `test_scene_exercises_the_cull` asserts from the oracle's per-patch table that they give the
cull something to do. The per-wave counter exists on the pair path only, so the counts are checked at the two pair extents
(and the counter is checked untouched at 97x55).
"""
import numpy as np
import pytest
import torch

import light_bounds_scene as scene
import lights_oracle as lo
import views
from helpers import f16_close, tol_units

pytestmark = pytest.mark.gpu
DEV = "cuda"
EXTENTS = [(64, 36), (98, 56), (97, 55)]
PAIR_EXTENTS = [(64, 36), (98, 56)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    return np.asarray(a).view(np.uint16)


_CASES = {}


def case(soc, W, H):
    """Inputs, device copies and the oracle's frame for one extent, made once."""
    if (W, H) not in _CASES:
        g, gb, ssao, clouds = scene.frame_inputs(W, H)
        host_ins = (gb["albedo"], gb["emissive"], gb["normal"], gb["depth"], ssao, gb["shadow"], clouds)
        ref, reach, lit = lo.composition(g, *host_ins, scene.POINT_RANGES, scene.SPOT_RANGES, subtexel_bits=8)
        dg = soc.globals_device_buffer()
        soc.upload_globals(g, dg)
        db = soc.light_bounds_device_buffer()
        soc.upload_light_bounds(soc.light_bounds(scene.POINT_RANGES, scene.SPOT_RANGES), db)
        _CASES[(W, H)] = dict(g=g, gb=gb, host_ins=host_ins, ins=[dev(a) for a in host_ins], ref=ref, reach=reach, lit=lit,
                              dg=dg, db=db)
    return _CASES[(W, H)]


def run(soc, c, W, H, fused=False, ins=None, out=None, **kw):
    out = torch.zeros(H, W, 4, dtype=torch.float16, device=DEV) if out is None else out
    ins = c["ins"] if ins is None else ins
    if not fused:
        soc.composition(c["g"], out, *ins, d_globals=c["dg"], **kw)
        return out, None
    ae = soc.auto_exposure_buffer()
    soc.composition_luminance_histogram(c["g"], out, *ins, ae, soc.histogram_scratch(), d_globals=c["dg"], **kw)
    return out, ae


@pytest.mark.parametrize("W,H", PAIR_EXTENTS)
def test_scene_exercises_the_cull(soc, W, H):
    c = case(soc, W, H)
    reach, lit = c["reach"], c["lit"]
    per_light = reach[lit].sum(0)
    assert (per_light == 0).any(), per_light              # a light that reaches no patch
    assert (per_light == lit.sum()).any(), per_light      # a light that reaches every lit patch
    empty = 1.0 - reach[lit].mean()
    assert 0.2 <= empty <= 0.8, empty


@pytest.mark.parametrize("cull", [True, False])
@pytest.mark.parametrize("W,H", EXTENTS)
def test_against_the_oracle(soc, W, H, cull):
    """Every pixel within the RGBA16F tolerance test_composition holds the unbounded kernels to (helpers.f16_close)."""
    c = case(soc, W, H)
    got = host(run(soc, c, W, H, bounds=c["db"], cull=cull)[0])
    print(f"{W}x{H} cull={cull}: max |d| in tolerance units {np.nanmax(tol_units(got, c['ref'])):.3f}")
    ok = f16_close(got, c["ref"])
    assert ok.all(), (ok.mean(), np.argwhere(~ok)[:5])
    sky = c["gb"]["depth"] == 1.0
    assert np.array_equal(bits(got[sky]), bits(c["ref"][sky]))


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("W,H", EXTENTS)
def test_cull_is_bit_identical(soc, W, H, fused):
    c = case(soc, W, H)
    on, ae_on = run(soc, c, W, H, fused, bounds=c["db"], cull=True)
    off, ae_off = run(soc, c, W, H, fused, bounds=c["db"], cull=False)
    assert np.array_equal(bits(host(on)), bits(host(off)))
    if fused:
        assert np.array_equal(host(ae_on), host(ae_off))
        assert int(host(ae_on)[1:].sum()) == W * H
        plain = run(soc, c, W, H, False, bounds=c["db"], cull=True)[0]
        assert np.array_equal(bits(host(on)), bits(host(plain)))


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("W,H", PAIR_EXTENTS)
def test_shaded_pairs_are_conservative_and_fewer(soc, W, H, fused):
    """The lights the waves ran: with the cull at least the oracle's non-empty (patch, light) pairs (no tolerance: a
    missing pair is a light dropped from a pixel it reaches) and strictly fewer than without it, which is every light
    for every wave with a lit pixel. The counting kernels give the bits of the others."""
    c = case(soc, W, H)
    needed = int(c["reach"][c["lit"]].sum())
    lights = len(scene.POINTS) + len(scene.SPOTS)
    n_on = torch.zeros(1, dtype=torch.int32, device=DEV)
    n_off = torch.zeros(1, dtype=torch.int32, device=DEV)
    on = run(soc, c, W, H, fused, bounds=c["db"], cull=True, shaded_pairs=n_on)[0]
    off = run(soc, c, W, H, fused, bounds=c["db"], cull=False, shaded_pairs=n_off)[0]
    ref = run(soc, c, W, H, fused, bounds=c["db"], cull=True)[0]
    n_on, n_off = int(host(n_on)[0]), int(host(n_off)[0])
    print(f"{W}x{H} fused={fused}: needed {needed}, culled {n_on} ({n_on / needed:.3f} x), all {n_off}")
    assert n_off == int(c["lit"].sum()) * lights
    assert needed <= n_on < n_off
    assert np.array_equal(bits(host(on)), bits(host(ref))) and np.array_equal(bits(host(off)), bits(host(ref)))


def test_generic_path_leaves_the_counter(soc):
    W, H = 97, 55
    c = case(soc, W, H)
    n = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    run(soc, c, W, H, bounds=c["db"], cull=True, shaded_pairs=n)
    assert int(host(n)[0]) == 7


def test_more_than_64_lights_of_a_kind(soc):
    """100 point and 70 spot lights (seeded, ranged, every eighth unlimited): lane i tests lights i and i + 64, and the
    loops walk a second mask per kind. Against the oracle, cull against no cull, and the counter against the oracle's."""
    W, H = 98, 56
    g, gb, ssao, clouds = scene.frame_inputs(W, H)
    rng = np.random.default_rng(0x64)
    npl, nsl = 100, 70
    g.point_light_count, g.spot_light_count = npl, nsl
    pr, sr = [], []
    for i in range(npl):
        L = g.point_lights[i]
        L.position[:] = [rng.uniform(-15.0, -2.0), rng.uniform(0.3, 6.0), rng.uniform(-4.0, 4.0)]
        L.color[:] = rng.uniform(0.3, 1.0, 3).tolist()
        L.intensity = float(rng.uniform(0.1, 0.5))
        pr.append(0.0 if i % 8 == 7 else float(rng.uniform(1.5, 4.0)))
    for i in range(nsl):
        L = g.spot_lights[i]
        L.position[:] = [rng.uniform(-15.0, -2.0), rng.uniform(2.0, 7.0), rng.uniform(-4.0, 4.0)]
        L.direction[:] = [rng.uniform(-0.5, 0.5), -1.0, rng.uniform(-0.5, 0.5)]
        L.color[:] = rng.uniform(0.3, 1.0, 3).tolist()
        L.intensity = float(rng.uniform(0.1, 0.5))
        L.cut_off, L.outer_cut_off = 0.95, 0.8
        sr.append(0.0 if i % 8 == 7 else float(rng.uniform(2.0, 6.0)))
    host_ins = (gb["albedo"], gb["emissive"], gb["normal"], gb["depth"], ssao, gb["shadow"], clouds)
    ref, reach, lit = lo.composition(g, *host_ins, pr, sr, subtexel_bits=8)
    needed = int(reach[lit].sum())
    assert reach[lit][:, 64:npl].any() and reach[lit][:, npl + 64:].any()      # the second halves matter
    dg = soc.globals_device_buffer()
    soc.upload_globals(g, dg)
    db = soc.light_bounds_device_buffer()
    soc.upload_light_bounds(soc.light_bounds(pr, sr), db)
    c = dict(g=g, dg=dg, ins=[dev(a) for a in host_ins])
    n = torch.zeros(1, dtype=torch.int32, device=DEV)
    on = host(run(soc, c, W, H, True, bounds=db, cull=True, shaded_pairs=n)[0])
    off = host(run(soc, c, W, H, True, bounds=db, cull=False)[0])
    plain = host(run(soc, c, W, H, False, bounds=db, cull=True)[0])
    assert np.array_equal(bits(on), bits(off)) and np.array_equal(bits(on), bits(plain))
    ok = f16_close(on, ref)
    assert ok.all(), (ok.mean(), np.argwhere(~ok)[:5])
    n = int(host(n)[0])
    print(f"{npl} + {nsl} lights: needed {needed}, culled {n} ({n / needed:.3f} x), all {int(lit.sum()) * (npl + nsl)}")
    assert needed <= n < int(lit.sum()) * (npl + nsl)


# ranged lights only (no light reaches everywhere): the lights of the NaN test
RANGED_POINTS = [1, 2, 3, 5]
RANGED_SPOTS = [1, 3, 5]


def test_rejected_light_leaves_no_nan(soc):
    """A patch of normals scaled by 1.5 (the unnormalised acos argument leaves [-1, 1]: NaN, composition.inl:133) outside
    every light's range and cone: the bounded frame is finite there and has the bits of the frame without lights; the
    unbounded call on the same input is NaN there (NaN times a zero cone term or a small 1/d^2 is NaN)."""
    W, H = 98, 56
    g, gb, ssao, clouds = scene.frame_inputs(W, H)
    g.point_light_count, g.spot_light_count = len(RANGED_POINTS), len(RANGED_SPOTS)
    for j, i in enumerate(RANGED_POINTS):
        L, src = g.point_lights[j], scene.POINTS[i]
        L.position[:], L.color[:], L.intensity = src[0], src[1], src[2]
    for j, i in enumerate(RANGED_SPOTS):
        L, src = g.spot_lights[j], scene.SPOTS[i]
        L.position[:], L.direction[:], L.color[:], L.intensity = src[0], src[1], src[2], src[3]
        L.cut_off, L.outer_cut_off = src[4], src[5]
    pr = [0.6 * scene.POINT_RANGES[i] for i in RANGED_POINTS]     # shorter: a patch with free neighbours all round
    sr = [0.6 * scene.SPOT_RANGES[i] for i in RANGED_SPOTS]
    host_ins = (gb["albedo"], gb["emissive"], gb["normal"], gb["depth"], ssao, gb["shadow"], clouds)
    _, reach, lit = lo.composition(g, *host_ins, pr, sr, subtexel_bits=8)
    free = np.argwhere(lit & ~reach.any(-1))
    # a patch fully inside the image whose neighbours are out of reach too (the oracle's and the device's roundings of
    # a boundary may differ by a pixel)
    pick = None
    for py, px in free:
        y0, x0 = py * lo.PATCH_H, px * lo.PATCH_W
        nb = reach[max(py - 1, 0):py + 2, max(px - 1, 0):px + 2]
        if y0 + lo.PATCH_H <= H and x0 + lo.PATCH_W <= W and not nb.any() and (gb["depth"][y0:y0 + 8, x0:x0 + 16] != 1.0).all():
            pick = (y0, x0)
            break
    assert pick is not None, "no patch out of every light's reach: the lights of this test need another look"
    y0, x0 = pick
    block = (slice(y0, y0 + lo.PATCH_H), slice(x0, x0 + lo.PATCH_W))
    normal = gb["normal"].copy()
    scaled = normal[block].astype(np.float32)
    scaled[..., :3] *= 1.5
    normal[block] = scaled.astype(np.float16)
    ins = [dev(a) for a in (gb["albedo"], gb["emissive"], normal, gb["depth"], ssao, gb["shadow"], clouds)]
    dg = soc.globals_device_buffer()
    soc.upload_globals(g, dg)
    db = soc.light_bounds_device_buffer()
    soc.upload_light_bounds(soc.light_bounds(pr, sr), db)
    c = dict(g=g, dg=dg, ins=ins)
    unbounded = host(run(soc, c, W, H)[0]).astype(np.float32)
    assert np.isnan(unbounded[block][..., :3]).any()
    g0 = scene.frame_inputs(W, H)[0]
    g0.point_light_count = g0.spot_light_count = 0
    no_lights = host(run(soc, dict(g=g0, dg=None, ins=ins), W, H)[0])
    for cull in (True, False):
        got = host(run(soc, c, W, H, bounds=db, cull=cull)[0])
        assert np.isfinite(got[block].astype(np.float32)).all()
        assert np.array_equal(bits(got[block]), bits(no_lights[block]))
        assert not np.array_equal(bits(got), bits(no_lights))      # the lights do light other pixels


@pytest.mark.parametrize("W,H", EXTENTS)
def test_unlimited_point_lights_are_the_unbounded_call(soc, W, H):
    """All ranges 0 and no spot lights: soc_composition's bits, with and without the cull, fused or not."""
    c = dict(case(soc, W, H))
    g = scene.frame_inputs(W, H)[0]
    g.spot_light_count = 0
    dg = soc.globals_device_buffer()
    soc.upload_globals(g, dg)
    db = soc.light_bounds_device_buffer()
    soc.upload_light_bounds(soc.light_bounds(), db)
    c.update(g=g, dg=dg)
    ref = host(run(soc, c, W, H)[0])
    for cull in (True, False):
        assert np.array_equal(bits(host(run(soc, c, W, H, bounds=db, cull=cull)[0])), bits(ref))
    assert np.array_equal(bits(host(run(soc, c, W, H, True, bounds=db)[0])), bits(ref))


def _frame(soc, W, H, gb):
    fr = soc.alloc_frame(W, H, DEV, bloom_output=True)
    for k in ("albedo", "emissive", "normal", "velocity", "depth"):
        fr[k].copy_(torch.from_numpy(gb[k]))
    fr["shadow"] = torch.from_numpy(gb["shadow"]).to(DEV)
    fr["noise"].copy_(torch.from_numpy(gb["noise"]))
    return fr


@pytest.mark.parametrize("cull", [True, False])
def test_render_graph(soc, cull):
    """Two frames with Renderer.set_light_bounds, the record rewritten between them: each frame's colour has the bits of
    the stand-alone fused bounded call on the frame's own intermediates. After set_light_bounds(None) the frame equals
    that of a renderer that never had bounds."""
    W, H = 64, 36
    g, gb, _, _ = scene.frame_inputs(W, H)
    fr = _frame(soc, W, H, gb)
    r = soc.Renderer(fr)
    names = r.pass_names()
    db = soc.light_bounds_device_buffer()
    r.set_light_bounds(db, cull=cull)
    assert r.pass_names() == names
    halved = ([0.5 * v for v in scene.POINT_RANGES], [0.5 * v for v in scene.SPOT_RANGES])
    colours = []
    for ranges in ((scene.POINT_RANGES, scene.SPOT_RANGES), halved):
        soc.upload_light_bounds(soc.light_bounds(*ranges), db)
        r.execute(g)
        colour = host(fr["color"]).copy()
        out = torch.zeros(H, W, 4, dtype=torch.float16, device=DEV)
        soc.composition_luminance_histogram(g, out, fr["albedo"], fr["bloom_output"], fr["normal"], fr["depth"],
                                            fr["ssao_blur"], fr["shadow"], fr["clouds"], soc.auto_exposure_buffer(),
                                            soc.histogram_scratch(), d_globals=fr["d_globals"], bounds=db, cull=cull)
        assert np.array_equal(bits(colour), bits(host(out)))
        colours.append(colour)
    assert not np.array_equal(bits(colours[0]), bits(colours[1]))
    r.set_light_bounds(None)
    r.execute(g)
    after = host(fr["color"]).copy()
    fr2 = _frame(soc, W, H, gb)
    r2 = soc.Renderer(fr2)
    r2.execute(g)
    assert np.array_equal(bits(after), bits(host(fr2["color"])))
    assert not np.array_equal(bits(after), bits(colours[0]))
    r.close()
    r2.close()


@pytest.mark.parametrize("fused", [False, True])
def test_padded_offset_views(soc, fused):
    """One bounded call on a padded, offset target and G-buffer (16-byte aligned rows: the pair path, with the cull)
    gives the contiguous call's bits and leaves the padding alone."""
    W, H = 98, 56
    c = case(soc, W, H)
    ref, ae_ref = run(soc, c, W, H, fused, bounds=c["db"])
    padded = []
    for i, t in enumerate(c["ins"]):
        v, canvas = views.make_view(t, "pad16", i) if i < 4 else (t, None)
        padded.append(v)
    out, canvas = views.make_view(torch.zeros(H, W, 4, dtype=torch.float16, device=DEV), "pad16", 7, role="out")
    got, ae = run(soc, c, W, H, fused, ins=padded, out=out, bounds=c["db"])
    assert np.array_equal(bits(host(got.contiguous())), bits(host(ref)))
    views.assert_padding_intact(canvas, H, W, "pad16", "target")
    if fused:
        assert np.array_equal(host(ae), host(ae_ref))
