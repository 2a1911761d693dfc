"""Cascaded sun shadow maps on the GPU (soc_composition_cascaded, soc_composition_luminance_histogram_cascaded,
soc_renderer_set_sun_cascades) against tests/cascades_oracle.py.

Extents: 64x36 (the pair path with a partial last tile row), 98x56 (partial tiles on both axes) and 97x55 (odd width:
composition_generic_cascaded). The frame is the C4 terrain (sun_cascades_scene.py), the records are
fit(count, S = 128, near = 16, max_distance = 104) with (count, lambda) = (3, 0.7) and (4, 0.5), every slab rasterised on
the host with its cascade's matrix. The scene check (every cascade selected by >= 3 % of the lit pixels, >= 4 pure and
>= 4 mixed 16 x 8 patches) is asserted from the oracle's selection inside the oracle comparison.
"""
import numpy as np
import pytest
import torch

import cascades_oracle as co
import sun_cascades_scene as scene
import views
from helpers import TERRAIN_CAMERA, f16_close, globals_for, tol_units
from soc_real_time_renderer_amd import raster
from soc_real_time_renderer_amd import scene as synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = scene.S


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    return np.asarray(a).view(np.uint16)


_CASES = {}


def case(soc, W, H, count, lam, lights=False):
    """Globals, record, atlas, device inputs and the oracle's frame of one (extent, record, lights), made once."""
    key = (W, H, count, lam, lights)
    if key not in _CASES:
        g0, gb, ssao, clouds = scene.frame_inputs(W, H)
        g = scene.copy_globals(g0)
        if lights:
            scene.set_lights(g)
        rec = scene.fit(g, count, lam)
        atlas = scene.atlas(g, rec)
        host_ins = scene.host_inputs(gb, ssao, clouds, atlas)
        ref, k, kinds = co.composition(g, *host_ins, rec, subtexel_bits=8)
        dg = soc.globals_device_buffer()
        soc.upload_globals(g, dg)
        _CASES[key] = dict(g=g, gb=gb, rec=rec, atlas=atlas, host_ins=host_ins, ins=[dev(a) for a in host_ins], ref=ref,
                           k=k, kinds=kinds, dg=dg)
    return _CASES[key]


def run(soc, c, W, H, fused=False, ins=None, out=None, rec="case", g=None):
    out = torch.zeros(H, W, 4, dtype=torch.float16, device=DEV) if out is None else out
    ins = c["ins"] if ins is None else ins
    rec = c["rec"] if isinstance(rec, str) else rec
    g = c["g"] if g is None else g
    if not fused:
        soc.composition(g, out, *ins, d_globals=c["dg"], cascades=rec)
        return out, None
    ae = soc.auto_exposure_buffer()
    soc.composition_luminance_histogram(g, out, *ins, ae, soc.histogram_scratch(), d_globals=c["dg"], cascades=rec)
    return out, ae


@pytest.mark.parametrize("lights", [False, True])
@pytest.mark.parametrize("count,lam", scene.RECORDS)
@pytest.mark.parametrize("W,H", scene.EXTENTS)
def test_against_the_oracle(soc, W, H, count, lam, lights):
    """Every pixel within the project's RGBA16F bound (helpers.f16_close, defaults); sky pixels bit-equal."""
    c = case(soc, W, H, count, lam, lights)
    shares, pure, mixed = scene.assert_scene(c["k"], c["kinds"], c["gb"]["depth"], count)
    got = host(run(soc, c, W, H)[0])
    units = tol_units(got, c["ref"])
    y, x, ch = np.unravel_index(np.nanargmax(units), units.shape)
    print(f"{W}x{H} count={count} lights={lights}: shares {np.round(shares, 3)}, pure {pure}, mixed {mixed}; worst pixel "
          f"({x}, {y}) channel {ch}: {units[y, x, ch]:.3f} tolerance units, cascade {c['k'][y, x]}; "
          f"{int((units > 1).any(-1).sum())} pixels over")
    ok = f16_close(got, c["ref"])
    assert ok.all(), (ok.mean(), np.argwhere(~ok)[:5])
    sky = c["gb"]["depth"] == 1.0
    assert sky.any() and np.array_equal(bits(got[sky]), bits(c["ref"][sky]))


@pytest.mark.parametrize("lights", [False, True])
@pytest.mark.parametrize("W,H", scene.EXTENTS)
def test_one_cascade_is_todays_call(soc, W, H, lights):
    """A record of the sun itself and the S x S map: soc_composition's bits; fused, the 256 bins as well. The cascaded
    kernels form the position in fp64, so this is a comparison of two roundings of one term, not the same
    instructions: it holds on these frames (measured: every pixel's bits equal at all three extents)."""
    g0, gb, ssao, clouds = scene.frame_inputs(W, H)
    g = scene.copy_globals(g0)
    if lights:
        scene.set_lights(g)
    dg = soc.globals_device_buffer()
    soc.upload_globals(g, dg)
    ins = [dev(a) for a in scene.host_inputs(gb, ssao, clouds, gb["shadow"])]
    rec = soc.sun_cascades_from_sun(g, S)
    c = dict(g=g, dg=dg, ins=ins, rec=rec)
    want = torch.zeros(H, W, 4, dtype=torch.float16, device=DEV)
    soc.composition(g, want, *ins, d_globals=dg)
    got = run(soc, c, W, H)[0]
    assert np.array_equal(bits(host(got)), bits(host(want)))
    ae_want = soc.auto_exposure_buffer()
    want_f = torch.zeros(H, W, 4, dtype=torch.float16, device=DEV)
    soc.composition_luminance_histogram(g, want_f, *ins, ae_want, soc.histogram_scratch(), d_globals=dg)
    got_f, ae = run(soc, c, W, H, fused=True)
    assert np.array_equal(bits(host(got_f)), bits(host(want_f)))
    assert np.array_equal(host(ae), host(ae_want))


@pytest.mark.parametrize("lights", [False, True])
@pytest.mark.parametrize("count,lam", scene.RECORDS)
def test_independent_of_the_wave(soc, count, lam, lights):
    """The 98x56 frame as it is, and with every sky pixel's depth replaced by a lit depth of the last cascade (pure
    patches at the horizon become mixed, sky patches become pure): every pixel whose own inputs did not change keeps its
    bits. Fused and unfused give the same colour bits, and the bins count every pixel."""
    W, H = 98, 56
    c = case(soc, W, H, count, lam, lights)
    rec = c["rec"]
    base, _ = run(soc, c, W, H)
    depth = c["gb"]["depth"]
    sky = depth == 1.0
    far = np.float32(0.5) * (np.float32(rec.split_depth[count - 2]) + np.float32(1.0))
    assert rec.split_depth[count - 2] < far < 1.0
    filled = depth.copy()
    filled[sky] = far
    k2 = co.select(filled, rec)
    kinds2 = co.patch_kinds(k2, np.ones_like(sky))
    assert (k2[sky] == count - 1).all()
    assert ((c["kinds"] == co.PURE) & (kinds2 == co.MIXED)).any()        # a pure patch turned mixed
    ins = list(c["ins"])
    ins[3] = dev(filled)
    other, _ = run(soc, c, W, H, ins=ins)
    base, other = host(base), host(other)
    assert np.array_equal(bits(base[~sky]), bits(other[~sky]))
    assert not np.array_equal(bits(base[sky]), bits(other[sky]))
    for these in (c["ins"], ins):
        plain = host(run(soc, c, W, H, ins=these)[0])
        fused, ae = run(soc, c, W, H, fused=True, ins=these)
        assert np.array_equal(bits(host(fused)), bits(plain))
        assert int(host(ae)[1:].sum()) == W * H


@pytest.mark.parametrize("W,H", scene.EXTENTS)
def test_slab_isolation(soc, W, H):
    """Slab 1's first and last rows set to 0.0: the pixels that select a neighbouring cascade keep their bits (a tap
    clamped to a slab's edge never reads the slab beside it), and the change is seen by slab 1's own pixels."""
    count, lam = scene.RECORDS[0]
    c = case(soc, W, H, count, lam)
    base = host(run(soc, c, W, H)[0])
    spoiled = c["atlas"].copy()
    spoiled[S] = spoiled[2 * S - 1] = 0.0
    ins = list(c["ins"])
    ins[5] = dev(spoiled)
    got = host(run(soc, c, W, H, ins=ins)[0])
    others = c["k"] != 1
    assert np.array_equal(bits(got[others]), bits(base[others]))
    ref = co.composition(c["g"], *scene.host_inputs(c["gb"], c["host_ins"][4], c["host_ins"][6], spoiled), c["rec"],
                         subtexel_bits=8)[0]
    assert f16_close(got, ref).all()


@pytest.mark.parametrize("fused", [False, True])
def test_padded_offset_views(soc, fused):
    """A padded, offset target and G-buffer (16-byte aligned rows: the pair path) and an atlas whose row pitch is wider
    than S give the contiguous call's bits and leave the padding alone."""
    W, H = 98, 56
    count, lam = scene.RECORDS[1]
    c = case(soc, W, H, count, lam, lights=True)
    ref, ae_ref = run(soc, c, W, H, fused)
    padded = []
    for i, t in enumerate(c["ins"]):
        v, _ = views.make_view(t, "pad16", i) if i < 4 or i == 5 else (t, None)
        padded.append(v)
    assert padded[5].stride(0) > S
    out, canvas = views.make_view(torch.zeros(H, W, 4, dtype=torch.float16, device=DEV), "pad16", 7, role="out")
    got, ae = run(soc, c, W, H, fused, ins=padded, out=out)
    assert np.array_equal(bits(host(got.contiguous())), bits(host(ref)))
    views.assert_padding_intact(canvas, H, W, "pad16", "target")
    if fused:
        assert np.array_equal(host(ae), host(ae_ref))


def _frame(soc, W, H, shadow_shape):
    fr = soc.alloc_frame(W, H, DEV, bloom_output=True)
    fr["noise"].copy_(torch.from_numpy(synth.noise_texture()))
    fr["shadow"] = torch.zeros(shadow_shape, dtype=torch.float32, device=DEV)
    return fr


def test_render_graph(soc):
    """A renderer over the terrain mesh as its raster scene with shadow = 1 and a count-3 atlas: set_sun_cascades leaves
    the pass names alone; after execute every slab has the bits of a stand-alone raster_depth with the cascade's matrix,
    and the colour those of the stand-alone fused cascaded call on the frame's own intermediates; a refit for a moved
    camera gives another frame that matches again; after set_sun_cascades(None) the frame equals that of a renderer that
    never had cascades (over a shadow image of the same extent: a renderer's images are fixed at creation)."""
    W, H = 64, 36
    count, lam = scene.RECORDS[0]
    g = globals_for(W, H, camera=TERRAIN_CAMERA)
    sc = raster.scene_setup(g, synth.TERRAIN, tex_size=128)
    fr = _frame(soc, W, H, (count * S, S))
    vis = torch.zeros((H, W), dtype=torch.int64, device=DEV)
    r = soc.Renderer(fr)
    r.set_raster_scene(sc["mesh"], sc["materials"], sc["material_count"], vis, sc["workspace"], shadow=True)
    names = r.pass_names()
    assert "SunShadowDraw" in names
    colours = []
    pos, rot = TERRAIN_CAMERA
    for camera in (TERRAIN_CAMERA, ((pos[0] - 6.0, pos[1] + 2.0, pos[2] + 3.0), rot)):
        g = globals_for(W, H, camera=camera)
        rec = scene.fit(g, count, lam)
        r.set_sun_cascades(rec)
        assert r.pass_names() == names
        r.execute(g)
        got_atlas = host(fr["shadow"]).copy()
        want_atlas = soc.sun_cascade_atlas(rec, DEV)
        raster.sun_shadow_draw_cascades(sc["mesh"], rec, want_atlas, sc["workspace"])
        assert np.array_equal(got_atlas.view(np.uint32), host(want_atlas).view(np.uint32))
        for k in range(count):
            slab = torch.zeros((S, S), dtype=torch.float32, device=DEV)
            raster.raster_depth(sc["mesh"], list(rec.projection_view[k]), raster.CULL_BACK, slab, sc["workspace"],
                                raster.SHADOW_BIAS_CONSTANT, raster.SHADOW_BIAS_SLOPE)
            assert np.array_equal(got_atlas[k * S:(k + 1) * S].view(np.uint32), host(slab).view(np.uint32)), k
            assert (got_atlas[k * S:(k + 1) * S] < 1.0).any(), k          # the terrain was drawn into the slab
        colour = host(fr["color"]).copy()
        out = torch.zeros(H, W, 4, dtype=torch.float16, device=DEV)
        soc.composition_luminance_histogram(g, out, fr["albedo"], fr["bloom_output"], fr["normal"], fr["depth"],
                                            fr["ssao_blur"], fr["shadow"], fr["clouds"], soc.auto_exposure_buffer(),
                                            soc.histogram_scratch(), d_globals=fr["d_globals"], cascades=rec)
        assert np.array_equal(bits(colour), bits(host(out)))
        colours.append(colour)
    assert not np.array_equal(bits(colours[0]), bits(colours[1]))
    r.set_sun_cascades(None)
    assert r.pass_names() == names
    r.execute(g)
    after = host(fr["color"]).copy()
    fr2 = _frame(soc, W, H, (count * S, S))
    r2 = soc.Renderer(fr2)
    r2.set_raster_scene(sc["mesh"], sc["materials"], sc["material_count"], torch.zeros_like(vis), sc["workspace"], shadow=True)
    r2.execute(g)
    assert np.array_equal(bits(after), bits(host(fr2["color"])))
    assert np.array_equal(host(fr["shadow"]).view(np.uint32), host(fr2["shadow"]).view(np.uint32))
    r.close()
    r2.close()


def test_unsupported_combinations(soc):
    W, H = 64, 36
    g = globals_for(W, H, camera=TERRAIN_CAMERA)
    rec = scene.fit(g, 3, 0.7)
    fr = _frame(soc, W, H, (3 * S, S))
    r = soc.Renderer(fr)
    db = soc.light_bounds_device_buffer()
    soc.upload_light_bounds(soc.light_bounds([4.0]), db)
    r.set_light_bounds(db)
    with pytest.raises(soc.SocError) as e:
        r.set_sun_cascades(rec)
    assert e.value.rc == -4 and "bounded lights" in str(e.value)
    r.set_light_bounds(None)
    r.set_sun_cascades(rec)
    r.set_light_bounds(db)                      # bounds set after the cascades: refused at execute
    with pytest.raises(soc.SocError) as e:
        r.execute(g)
    assert e.value.rc == -4 and "bounded lights" in str(e.value)
    r.close()
    rb = soc.Renderer(_frame(soc, W, H, (3 * S, S)), bloom_in_composition=True)
    with pytest.raises(soc.SocError) as e:
        rb.set_sun_cascades(rec)
    assert e.value.rc == -4 and "BLOOM_IN_COMPOSITION" in str(e.value)
    rb.close()
    # a shadow image that is not the record's atlas
    rs = soc.Renderer(_frame(soc, W, H, (S, S)))
    with pytest.raises(soc.SocError) as e:
        rs.set_sun_cascades(rec)
    assert e.value.rc == -1 and "atlas" in str(e.value)
    rs.close()
    # the stand-alone calls: cascades with bounds
    c = case(soc, W, H, 3, 0.7)
    out = torch.zeros(H, W, 4, dtype=torch.float16, device=DEV)
    with pytest.raises(ValueError):
        soc.composition(c["g"], out, *c["ins"], d_globals=c["dg"], cascades=c["rec"], bounds=db)
