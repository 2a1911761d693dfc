"""Every pass on padded, offset and misaligned image views (-m gpu).

Each entry point runs once on tight tensors and once per layout of tests/views.py (pad16, odd, mixed) with EVERY image
argument a view into a poisoned canvas, and each case asserts
  (a) the output views hold the tight run's bits (histogram bins, exposure, auxiliary images included),
  (b) every byte of every output canvas outside the view still holds the poison (a pass writes only inside its rows),
  (c) every input canvas is bit-identical to what it held before the call.
Input canvases are poisoned with NaN (0xA5 for uint8): a padding texel that reaches an output, even with weight zero,
changes its bits. The tight run is the one the existing parity tests check against the C oracle at these shapes; where no
existing test does (noted at the case), the tight run is compared with the oracle here, at that pass's existing bound.

The paths reached, from the dispatch code (tight = pad16 unless noted; "odd" also stands for the odd-indexed images of
mixed, whose calls take the unaligned side as soon as one gated image is unaligned):

  soc_bloom_downsample / _upsample (bloom.hip launch_bloom_down / _up): equal extents -> bloom_down_same_q /
      bloom_up_same_q, quad-row stores as 16-B pairs (pad16) or per texel (odd: vec16(dst) false); 2:1 ->
      bloom_down_half_w, 1:2 -> bloom_up_double (below 2^20 pixels), neither gated; 97x55 -> 48x27: the generic kernels.
      soc_bloom_chain is these eight launches: every mip has its own pitch.
  soc_bloom_weighted_stage (bloom_w.hip launch_bloom_weighted): bloomw_down01p<1>, bloomw_down23<true>, bloomw_up10r take
      no gate (8-B texel accesses at data % 16 == 8 in odd); bloomw_up32s<true> gets a16(mips[1]) false in odd (store2's
      scalar branch); with SOC_BLOOM_UP10_REG=0 bloomw_up10s gets a16(output) false in odd. An all-zero emissive takes
      the zero-skip stores of down01p / up10r / up10s.
  soc_ssao_generation (ssao.hip): no alignment gate; with the table ssao_pipe_kernel (the LDS tile staged by 16-B buffer
      loads at data % 8 == 4 in odd), SOC_SSAO_TILE=0 ssao_kernel<true, true, true>, without the table
      ssao_kernel<false, true, true>. The buffer resource spans pitch * height bytes of the view.
  soc_ssao_blur: ssao_blur_kernel, no gate (odd pitch and base in odd).
  soc_cloud_rendering (clouds.hip): clouds_classify's vec_store is target % 16 (pad16 1, odd 0); clouds_od_lut<R8 / RGBA8>
      reads the padded noise view; with and without the workspace (the pair lists / the single-lane kernel).
  soc_composition (composition_plan.cpp plan_composition): pad16 composition_pair<.., 7> (lights: <false, true>); odd and
      mixed composition_generic at even widths (composition_pair_path: aligned16 / depth & 7 fail; with lights: LIT_GENERIC_RELAXED). soc_composition_luminance_histogram: pad16
      the fused pair kernel + histogram_fold; odd / mixed the two-pass fallback (composition_generic, then the histogram).
  soc_generate_luminance_histogram (exposure.hip): 64x36 pad16 histogram_chunks, odd histogram_pixels at W % 8 == 0;
      97x55 histogram_pixels everywhere.
  soc_temporal_antialiasing[_tone_mapping] (taa.hip taa_launch): pad16 at even widths taa_lds<tm, rows, true> (fused
      RGBA8 store when the output is 8-B aligned); odd / mixed taa_fast and the separate tone map
      (tonemap_generic / tonemap_pair by its own gate); 100x40: a partial LDS tile row, 102x42: W % 4 == 2, H % 4 == 2.
  soc_tone_mapping (tonemap.hip): 64x36 pad16 tonemap_pair<FMT>, odd tonemap_generic<FMT> at an even width; 97x55 generic.
  soc_copy_image (taa.hip): pad16 copy_rows (16-B chunks and a byte tail), odd / mixed hipMemcpy2DAsync. soc_read_image:
      hipMemcpy2DAsync with the view's pitch.
  soc_raster_depth (raster.hip): raster_clear_depth (the width texels of each row), raster_small / raster_big with the
      view's pitch. soc_gbuffer_resolve: per-texel stores through each image's own pitch; level-0-only materials read
      padded texture views, mip-mapped ones padded level 0s with the chain of soc_generate_mips behind them and the
      paired texels of soc_pair_textures.
  soc_generate_mips / soc_pair_textures (texture.hip): level 1 from the padded level 0 by its pitch, the rest tight.
  soc_height_to_normal, soc_terrain_tessellate (terrain.hip), soc_generate_hiz (hiz.hip): no gates; every Hi-Z mip a view.
  Render graph: the frame's images all views (own index each); default flags and SKY_LANE_HIGH | BLOOM_IN_COMPOSITION,
      and the raster head writing the G-buffer and the shadow map into views. pad16 and mixed (the gated images at even
      indices) stay on the frame's fast paths (weighted bloom, composition_pair + histogram, sky_compose_pair, taa_lds with
      the fused store); odd takes composition_generic, the two-pass histogram, taa_fast and the separate tone map.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import views
from helpers import (SPONZA_CAMERA, f16_close, globals_for, random_rgba16, set_lights, sponza_inputs)
from soc_real_time_renderer_amd import raster, scene
from views import LAYOUTS, assert_padding_intact, bits_equal, make_view

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return np.ascontiguousarray(t.cpu().numpy())


class Views:
    """The images of one call under a layout: every image gets the next index (so in `mixed` no two share a pitch);
    check() asserts (b) on the outputs' canvases and (c) on the inputs'."""

    def __init__(self, layout):
        self.layout, self.n, self.ins, self.outs = layout, 0, [], []

    def _make(self, t, role, index=None):
        if index is None:
            index, self.n = self.n, self.n + 1
        return make_view(t, self.layout, index, role)

    def inp(self, t, name="input"):
        v, c = self._make(t, "in")
        if c is not None:
            self.ins.append((name, c, None))
        return v

    def out(self, t, name="output"):
        v, c = self._make(t, "out")
        if c is not None:
            self.outs.append((name, v, c))
        return v

    def inout(self, t, name="in/out", index=None):
        """An image the call reads and writes (the in-place bloom's emissive): NaN padding, checked as an output."""
        v, c = self._make(t, "in", index)
        if c is not None:
            self.outs.append((name, v, c))
        return v

    def freeze(self):
        """Snapshot the input canvases (after the inputs are filled, before the call)."""
        self.ins = [(n, c, c.clone()) for n, c, _ in self.ins]

    def check(self):
        torch.cuda.synchronize()
        for name, v, c in self.outs:
            assert_padding_intact(c, int(v.shape[0]), int(v.shape[1]), self.layout, name)
        for name, c, snap in self.ins:
            assert snap is not None, "freeze() before the call"
            assert bits_equal(c, snap), f"input canvas {name} changed ({self.layout})"


def run_layout(run, layout, relaxed=()):
    """run(vw) -> {name: output tensor}; asserts (a), (b), (c) of `layout` against the tight run, returns the tight
    run's outputs. `relaxed`: outputs of a pair of paths that legitimately differs, which the caller bounds instead."""
    tight = run(Views("tight"))
    torch.cuda.synchronize()
    tight = {k: v.clone() for k, v in tight.items()}
    vw = Views(layout)
    got = run(vw)
    vw.check()
    differ = {k: _mismatch(got[k], tight[k]) for k in tight if k not in relaxed and not bits_equal(got[k], tight[k])}
    assert not differ, (layout, differ)
    return tight


def _mismatch(a, b):
    if a.shape != b.shape:
        return (tuple(a.shape), tuple(b.shape))
    d = (views._int_bits(a.contiguous()) != views._int_bits(b.contiguous()))
    if d.dim() == 3:
        d = d.any(dim=2)
    idx = torch.nonzero(d)
    return int(d.sum()), idx[:5].tolist()


_ONCE = {}


def once(key, fn):
    """Oracle comparisons of a tight run: once per case, not per layout."""
    if key not in _ONCE:
        _ONCE[key] = True
        fn()


def f16z(H, W, fill=0.0):
    return torch.full((H, W, 4), fill, dtype=torch.float16, device=DEV)


# ------------------------------------------------------------------------------------------------ bloom
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("W,H", [(64, 36), (97, 55)])
def test_bloom_passes(soc, oracle, W, H, layout):
    """The source / target pairs of test_bloom_passes_bit_exact (which checks the tight runs against the oracle)."""
    g = globals_for(W, H)
    dims = [(max(W >> i, 1), max(H >> i, 1)) for i in range(4)]
    cases = [(0, (W, H), dims[0], 7), (0, dims[0], dims[1], 7), (0, dims[1], dims[2], 7),
             (1, dims[1], dims[0], 3), (1, dims[0], (W, H), 3), (1, dims[3], dims[2], 3)]
    for up, (sw, sh), (dw, dh), k in cases:
        s = dev(random_rgba16(sh, sw, seed=sw * k + sh))

        def run(vw):
            src, out = vw.inp(s, "source"), vw.out(f16z(dh, dw), "target")
            vw.freeze()
            (soc.bloom_upsample if up else soc.bloom_downsample)(g, src, out)
            return {"target": out}
        run_layout(run, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("W,H", [(64, 36), (97, 55)])
def test_bloom_chain(soc, oracle, W, H, layout):
    """97x55 is not a shape of test_bloom_chain_bit_exact: the tight run against the oracle here (bit-exact rgb)."""
    g = globals_for(W, H)
    em = random_rgba16(H, W, seed=5, hi=8.0)
    shapes = [(max(H >> i, 1), max(W >> i, 1)) for i in range(4)]

    def run(vw):
        e = vw.inout(dev(em), "emissive")
        mips = [vw.out(f16z(h, w), f"mip{i}") for i, (h, w) in enumerate(shapes)]
        vw.freeze()
        soc.bloom_chain(g, e, mips)
        return dict({"emissive": e}, **{f"mip{i}": m for i, m in enumerate(mips)})
    tight = run_layout(run, layout)

    def against_oracle():
        em_h = em.copy()
        mips_h = [np.zeros((h, w, 4), np.float16) for h, w in shapes]
        oracle.bloom_chain(g, em_h, mips_h)
        assert np.array_equal(host(tight["emissive"])[..., :3].view(np.uint16), em_h[..., :3].view(np.uint16))
        for i in range(4):
            assert np.array_equal(host(tight[f"mip{i}"])[..., :3].view(np.uint16), mips_h[i][..., :3].view(np.uint16)), i
    once(("bloom_chain", W, H), against_oracle)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("emissive", ["dense", "zero"])
@pytest.mark.parametrize("up10_reg", ["1", "0"])
@pytest.mark.parametrize("W,H", [(64, 40), (136, 40)])
def test_bloom_weighted_stage(soc, monkeypatch, W, H, up10_reg, emissive, layout):
    """Stage 0, stages 1 to 4 one by one, and the in-place form (output = the emissive view). The dense tight run
    against the eight separate passes (bit-exact to the oracle) within the RGBA16F tolerance, as
    test_bloom_weighted_chain bounds it."""
    monkeypatch.setenv("SOC_BLOOM_UP10_REG", up10_reg)
    soc.reload_tuning()
    g = globals_for(W, H)
    em = random_rgba16(H, W, seed=23, hi=16.0) if emissive == "dense" else np.zeros((H, W, 4), np.float16)
    shapes = [(H >> i, W >> i) for i in range(4)]

    def make(form):
        def run(vw):
            e = (vw.inout if form == "in_place" else vw.inp)(dev(em), "emissive")
            mips = [vw.out(f16z(h, w, 7.0), f"mip{i}") for i, (h, w) in enumerate(shapes)]
            out = e if form == "in_place" else vw.out(f16z(H, W, 7.0), "output")
            vw.freeze()
            for st in ((1, 2, 3, 4) if form == "stages" else (0,)):
                soc.bloom_weighted_stage(g, e, mips, out, st)
            return {"output": out, "mip0": mips[0], "mip1": mips[1], "mip2": mips[2], "mip3": mips[3]}
        return run
    tights = {form: run_layout(make(form), layout) for form in ("all", "stages", "in_place")}
    for form in ("stages", "in_place"):
        for k in ("output", "mip1", "mip3"):
            assert bits_equal(tights[form][k], tights["all"][k]), (form, k)
    assert torch.all(tights["all"]["mip0"] == 7.0) and torch.all(tights["all"]["mip2"] == 7.0)   # scratch: not written

    def against_separate_passes():
        e = dev(em)
        ref = [f16z(h, w) for h, w in shapes]
        ref_out = f16z(H, W)
        soc.bloom_downsample(g, e, ref[0])
        for i in range(3):
            soc.bloom_downsample(g, ref[i], ref[i + 1])
        ref3 = ref[3].clone()
        for i in range(3, 0, -1):
            soc.bloom_upsample(g, ref[i], ref[i - 1])
        soc.bloom_upsample(g, ref[0], ref_out)
        for got, want in ((tights["all"]["output"], ref_out), (tights["all"]["mip1"], ref[1]),
                          (tights["all"]["mip3"], ref3)):
            assert f16_close(host(got)[..., :3], host(want)[..., :3]).all()
    once(("bloom_w", W, H, up10_reg, emissive), against_separate_passes)


# ------------------------------------------------------------------------------------------------ ssao
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("variant", ["table", "table_gather", "no_table"])
@pytest.mark.parametrize("W,H", [(128, 72), (97, 55)])
def test_ssao_generation(soc, monkeypatch, W, H, variant, layout):
    """The shapes and inputs of test_ssao_generation (tight against the oracle there); the table variants against the
    no-table kernel by test_ssao_noise_table_is_bit_identical / test_ssao_tile_orders_bit_identical."""
    if variant == "table_gather":
        monkeypatch.setenv("SOC_SSAO_TILE", "0")
        soc.reload_tuning()
    g, gb = sponza_inputs(W, H)
    hh, hw = H // 2, W // 2

    def run(vw):
        depth, normal = vw.inp(dev(gb["depth"]), "depth"), vw.inp(dev(gb["normal"]), "normal")
        out = vw.out(torch.zeros(hh, hw, dtype=torch.uint8, device=DEV), "target")
        table = None
        if variant != "no_table":
            table = torch.zeros(hh * hw * 2, dtype=torch.float32, device=DEV)
            soc.ssao_prepare_noise(normal, out, table)
        vw.freeze()
        soc.ssao_generation(g, depth, normal, out, table)
        return {"target": out}
    run_layout(run, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("W,H", [(100, 40), (16, 8)])
def test_ssao_blur(soc, W, H, layout):
    """Shapes and input of test_ssao_blur_bit_exact."""
    g = globals_for(W, H)
    src = np.random.default_rng(3).integers(0, 256, (H // 2, W // 2), dtype=np.uint8)

    def run(vw):
        s = vw.inp(dev(src), "ssao")
        out = vw.out(torch.zeros(H // 2, W // 2, dtype=torch.uint8, device=DEV), "target")
        vw.freeze()
        soc.ssao_blur(g, s, out)
        return {"target": out}
    run_layout(run, layout)


# ------------------------------------------------------------------------------------------------ clouds
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("noise_format", ["rgba8", "r8"])
@pytest.mark.parametrize("workspace", [False, True])
def test_cloud_rendering(soc, oracle, workspace, noise_format, layout):
    """96x64, the inputs of test_clouds (tight RGBA8 noise against the oracle there; the R8 noise holds the same red
    channel: its tight run must equal the RGBA8 one, as test_clouds_pair_path_equals_single_lane states)."""
    W, H = 96, 64
    g, gb = sponza_inputs(W, H, camera=((-14.0, 2.2, 0.3), (0.0, -0.42, 0.0)), elapsed=10.0)
    noise = gb["noise"] if noise_format == "rgba8" else np.ascontiguousarray(gb["noise"][..., 0])

    def run(vw):
        depth, nz = vw.inp(dev(gb["depth"]), "depth"), vw.inp(dev(noise), "noise")
        out = vw.out(torch.zeros(H, W, 4, dtype=torch.uint8, device=DEV), "target")
        ws = soc.cloud_rendering_workspace(W, H) if workspace else None
        vw.freeze()
        soc.cloud_rendering(g, depth, nz, out, ws)
        return {"target": out}
    tight = run_layout(run, layout)

    def against_oracle():
        ref = np.zeros((H, W, 4), np.uint8)
        oracle.cloud_rendering(g, gb["depth"], gb["noise"], ref)
        d = np.abs(host(tight["target"]).astype(np.int32) - ref.astype(np.int32))
        assert (d <= 2).mean() >= 0.995, ((d <= 2).mean(), d.max())
    once(("clouds", workspace, noise_format), against_oracle)


# ------------------------------------------------------------------------------------------------ composition
def _composition_inputs(W, H, lights):
    g, gb = sponza_inputs(W, H, elapsed=10.0)
    rng = np.random.default_rng(W + lights)
    gb["ssao"] = rng.integers(120, 256, (H // 2, W // 2), dtype=np.uint8)
    gb["clouds"] = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    set_lights(g, lights, lights)
    return g, gb


COMP_KEYS = ("albedo", "emissive", "normal", "depth", "ssao", "shadow", "clouds")

# With point / spot lights, composition_pair (tight, pad16) runs the light loops on a lane's two pixels as packed f32
# pairs (light_sum<f2v>) and composition_generic (odd, mixed) per pixel (light_sum<float>). The file is compiled with the
# compiler's implicit contraction, which fuses different multiply-add pairs in the two forms and around them: measured,
# one pixel of 64x36 and two of 98x56 differ in the last RGBA16F bit (with every fma of the loops pinned by a contract(off)
# pragma a different pixel; no variant tried made them equal). No identity test claims the two kernels' bits equal with
# lights; both are within the pass's oracle bound. For the lit odd / mixed cases (a) is therefore that bound,
# helpers.f16_close against the oracle on every value, as test_composition asserts it; without lights the bits are equal.
LIT_GENERIC_RELAXED = ("target",)


def _composition_bound(oracle, g, gb, W, H, target, label):
    ref = np.zeros((H, W, 4), np.float16)
    oracle.composition(g, ref, *[gb[k] for k in COMP_KEYS])
    ok = f16_close(host(target), ref)
    assert ok.all(), (label, ok.mean(), np.argwhere(~ok)[:5])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("lights", [0, 3])
@pytest.mark.parametrize("W,H", [(64, 36), (98, 56)])
def test_composition(soc, oracle, W, H, lights, layout):
    """The tight run against the oracle here (98x56 and these lights are not cases of test_composition), at its bound.
    Lit odd / mixed cases: LIT_GENERIC_RELAXED."""
    g, gb = _composition_inputs(W, H, lights)
    dg = soc.globals_device_buffer()
    soc.upload_globals(g, dg)

    def run(vw):
        out = vw.out(f16z(H, W), "target")
        ins = [vw.inp(dev(gb[k]), k) for k in COMP_KEYS]
        vw.freeze()
        soc.composition(g, out, *ins, d_globals=dg)
        if vw.layout != "tight" and lights:
            _composition_bound(oracle, g, gb, W, H, out, vw.layout)
        return {"target": out}
    tight = run_layout(run, layout, relaxed=LIT_GENERIC_RELAXED if lights and layout != "pad16" else ())
    once(("composition", W, H, lights), lambda: _composition_bound(oracle, g, gb, W, H, tight["target"], "tight"))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("lights", [0, 3])
@pytest.mark.parametrize("W,H", [(64, 36), (98, 56)])
def test_composition_luminance_histogram(soc, oracle, W, H, lights, layout):
    """Colour and bins; the tight run's colour equals soc_composition's (checked against the oracle above) and its bins
    those of the histogram pass on it, as test_composition_histogram_fused states for these shapes."""
    g, gb = _composition_inputs(W, H, lights)
    dg = soc.globals_device_buffer()
    soc.upload_globals(g, dg)

    def run(vw):
        out = vw.out(f16z(H, W), "target")
        ins = [vw.inp(dev(gb[k]), k) for k in COMP_KEYS]
        ae = soc.auto_exposure_buffer()
        ae[1:] = 7
        scratch = soc.histogram_scratch()
        vw.freeze()
        soc.composition_luminance_histogram(g, out, *ins, ae, scratch, d_globals=dg)
        if vw.layout != "tight" and lights and vw.layout != "pad16":
            # LIT_GENERIC_RELAXED: the colour at the oracle bound; the bins must be those of the histogram pass on this
            # very colour (bit-exact against the oracle in test_histogram_bit_exact), as the two-pass fallback computes them
            _composition_bound(oracle, g, gb, W, H, out, vw.layout)
            a = soc.auto_exposure_buffer()
            a[1:] = 7
            soc.generate_luminance_histogram(g, out.contiguous(), a)
            torch.cuda.synchronize()
            assert torch.equal(a, ae), vw.layout
        return {"target": out, "bins": ae, "scratch": scratch}
    tight = run_layout(run, layout, relaxed=LIT_GENERIC_RELAXED + ("bins",) if lights and layout != "pad16" else ())

    def against_two_passes():
        c = f16z(H, W)
        soc.composition(g, c, *[dev(gb[k]) for k in COMP_KEYS], d_globals=dg)
        a = soc.auto_exposure_buffer()
        a[1:] = 7
        soc.generate_luminance_histogram(g, c, a)
        torch.cuda.synchronize()
        assert bits_equal(c, tight["target"]) and torch.equal(a, tight["bins"])
        assert int(tight["bins"][1:].sum()) == W * H + 7 * 256 and int(tight["scratch"].abs().sum()) == 0
    once(("composition_hist", W, H, lights), against_two_passes)


# ------------------------------------------------------------------------------------------------ exposure
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("W,H", [(64, 36), (97, 55)])
def test_generate_luminance_histogram(soc, W, H, layout):
    """Shapes and input of test_histogram_bit_exact."""
    g = globals_for(W, H)
    rng = np.random.default_rng(W)
    img = np.exp(rng.normal(-1.0, 3.0, (H, W, 4))).astype(np.float16)
    img[rng.uniform(size=(H, W)) < 0.05] = 0.0
    img[0, 0] = np.float16(np.nan)

    def run(vw):
        hdr = vw.inp(dev(img), "hdr")
        buf = soc.auto_exposure_buffer()
        vw.freeze()
        soc.generate_luminance_histogram(g, hdr, buf)
        return {"bins": buf}
    tight = run_layout(run, layout)
    assert int(tight["bins"][1:].sum()) == W * H


# ------------------------------------------------------------------------------------------------ TAA
def _taa_inputs(W, H):
    g, gb = sponza_inputs(W, H)
    pvel = gb["velocity"].copy()
    pvel[..., :2] += np.float16(0.0015)
    return g, {"cur": random_rgba16(H, W, seed=3, hi=3.0), "prev": random_rgba16(H, W, seed=4, hi=3.0),
               "vel": gb["velocity"], "pvel": pvel, "depth": gb["depth"]}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("W,H", [(64, 36), (100, 40), (102, 42)])
def test_temporal_antialiasing(soc, oracle, W, H, fused, layout):
    """The inputs of test_taa_lane_shift_neighbours_identical; the tight run against the oracle here (64x36 is not one of
    its shapes), at the RGBA16F bound; the fused framebuffer against the tone-map pass on the tight result within the
    bound of test_taa_tone_mapping_fused_equals_two_passes."""
    g, d = _taa_inputs(W, H)

    def run(vw):
        t = vw.out(f16z(H, W), "target")
        ins = [vw.inp(dev(d[k]), k) for k in ("cur", "prev", "vel", "pvel", "depth")]
        vo = vw.out(f16z(H, W), "velocity_history_out")
        res = {"target": t, "velocity_history_out": vo}
        if fused:
            o = vw.out(torch.zeros(H, W, 4, dtype=torch.uint8, device=DEV), "output")
            ae = soc.auto_exposure_buffer(exposure=0.37)
            vw.freeze()
            soc.temporal_antialiasing_tone_mapping(g, t, *ins, ae, o, vo)
            res["output"] = o
        else:
            vw.freeze()
            soc.temporal_antialiasing(g, t, *ins, vo)
        return res
    if fused and layout != "pad16":
        # the fused launch (pad16: taa_lds storing the framebuffer) and the separate tone-map pass (odd, mixed: the pair
        # gate fails) legitimately differ by one level on < 1e-4 of the values (test_taa_tone_mapping_fused_equals_two_passes
        # bounds them so): the framebuffer against the tight run's within that bound, everything else bit for bit
        tight = run(Views("tight"))
        torch.cuda.synchronize()
        vw = Views(layout)
        got = run(vw)
        vw.check()
        for k in ("target", "velocity_history_out"):
            assert bits_equal(got[k], tight[k]), (layout, k, _mismatch(got[k], tight[k]))
        dd = (got["output"].int() - tight["output"].int()).abs()
        assert int(dd.max()) <= 1 and float((dd > 0).float().mean()) < 1e-4
    else:
        tight = run_layout(run, layout)
    assert bits_equal(tight["velocity_history_out"], dev(d["vel"]))

    def against_oracle():
        ref = np.zeros((H, W, 4), np.float16)
        oracle.temporal_antialiasing(g, ref, d["cur"], d["prev"], d["vel"], d["pvel"], d["depth"])
        ok = f16_close(host(tight["target"]), ref)
        assert ok.all(), ok.mean()
        if fused:
            o1 = torch.zeros(H, W, 4, dtype=torch.uint8, device=DEV)
            soc.tone_mapping(g, tight["target"], soc.auto_exposure_buffer(exposure=0.37), o1)
            dd = (o1.int() - tight["output"].int()).abs()
            assert int(dd.max()) <= 1 and float((dd > 0).float().mean()) < 1e-4
    once(("taa", W, H, fused), against_oracle)


# ------------------------------------------------------------------------------------------------ tone mapping
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fmt", ["RGBA8_UNORM", "RGBA8_SRGB", "RGBA32F"])
@pytest.mark.parametrize("W,H", [(64, 36), (97, 55)])
def test_tone_mapping(soc, W, H, fmt, layout):
    """Shapes, formats and input of test_tone_mapping."""
    g = globals_for(W, H)
    img = random_rgba16(H, W, seed=4, lo=-0.5, hi=6.0)
    F = getattr(soc, "FMT_" + fmt)

    def run(vw):
        color = vw.inp(dev(img), "color")
        out = vw.out(torch.zeros(H, W, 4, dtype=torch.float32 if fmt == "RGBA32F" else torch.uint8, device=DEV), "target")
        vw.freeze()
        soc.tone_mapping(g, color, soc.auto_exposure_buffer(exposure=-0.8), out, F)
        return {"target": out}
    run_layout(run, layout)


# ------------------------------------------------------------------------------------------------ copy / read
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("fmt", ["rgba16f", "r8"])
@pytest.mark.parametrize("W,H", [(64, 36), (97, 55)])
def test_copy_and_read_image(soc, W, H, fmt, layout):
    """No oracle: the copy of an image is the image (asserted on the tight run)."""
    rng = np.random.default_rng(W)
    src = random_rgba16(H, W, seed=9) if fmt == "rgba16f" else rng.integers(0, 256, (H, W), dtype=np.uint8)

    def run(vw):
        s = vw.inp(dev(src), "source")
        t = vw.out(torch.zeros_like(dev(src)), "target")
        vw.freeze()
        soc.copy_image(t, s)
        back = soc.read_image(t)
        return {"target": t, "read": torch.from_numpy(back), "read_source": torch.from_numpy(soc.read_image(s))}
    tight = run_layout(run, layout)
    for k in tight:
        assert bits_equal(tight[k].cpu(), torch.from_numpy(np.ascontiguousarray(src))), k


# ------------------------------------------------------------------------------------------------ raster
_SCENE = {}


def _proxy_scene(W, H):
    """The box-atrium mesh of test_gpu_raster.py (host and device) and the frame's globals."""
    if (W, H) not in _SCENE:
        g = globals_for(W, H, camera=SPONZA_CAMERA)
        m = scene.mesh(g, scene.SPONZA_PROXY)
        hm = raster.MeshBuffers(m["positions"], m["normals"], m["uvs"], m["indices"], m["materials"])
        dm = raster.MeshBuffers.from_numpy(m["positions"], m["normals"], m["uvs"], m["indices"], m["materials"])
        _SCENE[(W, H)] = (g, hm, dm)
    return _SCENE[(W, H)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("which", ["camera", "sun"])
def test_raster_depth(soc, oracle, which, layout):
    """97x55 depth-only raster: the camera's view (cull FRONT, no bias) and the sun's (cull BACK, the shadow bias). The
    tight run against the oracle here (bit-exact, as test_shadow_depth_bit_exact). Without the per-row clear (the clear
    of pitch / 4 * height dwords from the view's base) the 1.0f fill lands on the poison right of every row and in the
    lower guard rows: (b) fails."""
    W, H = 97, 55
    g, hm, dm = _proxy_scene(W, H)
    if which == "camera":
        vp, cull, bias = np.ctypeslib.as_array(g.camera_projection_view_matrix), raster.CULL_FRONT, (0.0, 0.0)
    else:
        vp, cull = np.ctypeslib.as_array(g.sun_info.projection_view_matrix), raster.CULL_BACK
        bias = (raster.SHADOW_BIAS_CONSTANT, raster.SHADOW_BIAS_SLOPE)
    ws = dm.workspace()

    def run(vw):
        d = vw.out(torch.zeros(H, W, dtype=torch.float32, device=DEV), "depth")
        vw.freeze()
        raster.raster_depth(dm, vp, cull, d, ws, *bias)
        return {"depth": d}
    tight = run_layout(run, layout)

    def against_oracle():
        ref = np.zeros((H, W), np.float32)
        oracle.raster_depth(hm, vp, cull, ref, *bias)
        assert np.array_equal(host(tight["depth"]).view(np.uint32), ref.view(np.uint32))
        assert (ref < 1.0).mean() > 0.05
    once(("raster_depth", which), against_oracle)


class PaddedMipTexture(raster.MipTexture):
    """A MipTexture whose level 0 is a padded view: one flat poisoned buffer holding G guard rows, the level-0 rows of
    (L + W + R) texels, the tight levels 1.. where the packed layout puts them (data + pitch * H) and a guard behind
    them. `written` marks the bytes soc_generate_mips may write (levels 1..)."""

    def __init__(self, level0, srgb, layout, index):
        H, W = int(level0.shape[0]), int(level0.shape[1])
        L, R = views._margins(W, 4, layout, index)
        self.pitch = (L + W + R) * 4
        self.offset = views.G * self.pitch + L * 4
        chain = int(raster.lib().soc_mip_chain_bytes(W, H, self.pitch))
        guard = views.G * self.pitch
        flat = torch.full((self.offset + chain + guard,), views.IN_POISON_U8, dtype=torch.uint8, device=DEV)
        rows = flat[views.G * self.pitch:(views.G + H) * self.pitch].view(H, L + W + R, 4)
        rows[:, L:L + W] = level0
        super().__init__(flat, W, H, srgb)
        self.level0 = rows[:, L:L + W]
        self.padding = torch.ones_like(flat, dtype=torch.bool)
        self.padding[views.G * self.pitch:(views.G + H) * self.pitch].view(H, L + W + R, 4)[:, L:L + W] = False
        self.padding[self.offset + self.pitch * H:self.offset + chain] = False

    def img(self):
        return soc_img(self.buf.data_ptr() + self.offset, self.width, self.height, self.pitch, self.format)

    def generate(self):
        raster._check(raster.lib().soc_generate_mips(self.img(), torch.cuda.current_stream().cuda_stream), "generate_mips")
        return self

    def upper_levels(self):
        """The bytes of levels 1.. (tight, packed)."""
        n = sum(h * w * 4 for h, w in raster.mip_level_shapes(self.width, self.height)[1:])
        start = self.offset + self.pitch * self.height
        return self.buf[start:start + n]

    def assert_padding_intact(self, what):
        bad = (self.buf != views.IN_POISON_U8) & self.padding
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} padding bytes of the mip-chain buffer were overwritten"


def soc_img(data, w, h, pitch, fmt):
    from soc_real_time_renderer_amd import SocImg
    return SocImg(data, w, h, pitch, fmt)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("W,H,srgb", [(64, 64, False), (64, 64, True), (48, 20, True)])
def test_generate_mips_and_pair_textures(soc, oracle, W, H, srgb, layout):
    """A padded level 0: levels 1.. equal the packed chain built from the tight level 0 (checked against the oracle
    here, bit-exact as test_generate_mips_bit_exact; 48x20 is not one of its shapes), the level 0 and the padding are
    untouched, and the paired texels of two padded chains equal those of the tight ones."""
    rng = np.random.default_rng(W * 1000 + H)
    l0a, l0n = (rng.integers(0, 256, (H, W, 4), dtype=np.uint8) for _ in range(2))
    ta, tn = raster.MipTexture.build(l0a, srgb, DEV), raster.MipTexture.build(l0n, False, DEV)
    pa = PaddedMipTexture(dev(l0a), srgb, layout, 0)
    pn = PaddedMipTexture(dev(l0n), False, layout, 1)
    before = pa.buf.clone()
    pa.generate()
    pn.generate()
    torch.cuda.synchronize()
    n0 = W * H * 4
    assert torch.equal(pa.upper_levels(), ta.buf[n0:]) and torch.equal(pn.upper_levels(), tn.buf[n0:])
    pa.assert_padding_intact("albedo chain")
    pn.assert_padding_intact("normal chain")
    assert torch.equal(pa.level0, dev(l0a)) and torch.equal(pa.buf[pa.padding], before[pa.padding])
    nbytes = int(soc.lib().soc_paired_texels_bytes(W, H))
    guard = 64
    bufs = []
    for a, n in ((ta, tn), (pa, pn)):
        buf = torch.full((nbytes + 2 * guard,), 0x5B, dtype=torch.uint8, device=DEV)
        snap = (a.buf.clone(), n.buf.clone())
        raster._check(soc.lib().soc_pair_textures(a.img(), n.img(), C.c_void_p(buf.data_ptr() + guard),
                                                  torch.cuda.current_stream().cuda_stream), "pair_textures")
        torch.cuda.synchronize()
        assert torch.equal(a.buf, snap[0]) and torch.equal(n.buf, snap[1])
        assert bool((buf[:guard] == 0x5B).all()) and bool((buf[guard + nbytes:] == 0x5B).all())
        bufs.append(buf)
    assert torch.equal(bufs[0], bufs[1])

    def against_oracle():
        buf = np.zeros(raster.MipTexture.chain_bytes(W, H), np.uint8)
        buf[:n0] = l0a.reshape(-1)
        ref = raster.MipTexture(buf, W, H, srgb)
        oracle.generate_mips(ref)
        for k, (a, b) in enumerate(zip(ta.levels(), ref.levels())):
            assert np.array_equal(a, b), k
    once(("mips", W, H, srgb), against_oracle)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mipmapped", [False, True])
def test_raster_visibility_and_gbuffer_resolve(soc, oracle, mipmapped, layout):
    """97x55 on the box atrium: depth and the four G-buffer targets are views, the material textures padded views
    (level 0 only) or padded level 0s with their generated chains and paired texels (mip-mapped, with a normal texture
    per material). The tight run against the oracle here at test_gbuffer_resolve's bound (depth bit-exact, RGBA16F
    within the tolerance)."""
    W, H = 97, 55
    g, hm, dm = _proxy_scene(W, H)
    vp = np.ctypeslib.as_array(g.camera_projection_view_matrix)
    tex, em = scene.material_textures(g, 32, scene.SPONZA_PROXY)
    rng = np.random.default_rng(17)
    nrm = [np.ascontiguousarray(np.concatenate([rng.integers(96, 160, (32, 32, 2), dtype=np.uint8),
                                                np.full((32, 32, 2), 255, np.uint8)], -1)) for _ in tex]
    ws = dm.workspace()
    vis = torch.zeros((H, W), dtype=torch.int64, device=DEV)
    raster.raster_visibility(dm, vp, raster.CULL_FRONT, vis, ws)
    kw = [dict(emissive_factor=tuple(float(v) for v in em[i]) + (1.0,), has_emissive=bool(em[i].any()))
          for i in range(len(tex))]

    def run(vw):
        keep, mats, alive = [], [], []      # a material holds addresses only: `alive` holds the textures until the sync
        for i in range(len(tex)):
            if mipmapped:
                if vw.layout == "tight":
                    a, n = raster.MipTexture.build(tex[i], True, DEV), raster.MipTexture.build(nrm[i], False, DEV)
                    alive += [a, n]
                else:
                    a = PaddedMipTexture(dev(tex[i]), True, vw.layout, 2 * i).generate()
                    n = PaddedMipTexture(dev(nrm[i]), False, vw.layout, 2 * i + 1).generate()
                    keep.append((a, a.buf.clone()))
                    keep.append((n, n.buf.clone()))
                mats.append(raster.material(albedo=a, normal_texture=n, **kw[i]))
                assert mats[-1].flags & raster.MATERIAL_PAIRED_TEXELS
            else:
                alive.append(vw.inp(dev(tex[i]), f"albedo texture {i}"))
                mats.append(raster.material(albedo=alive[-1], **kw[i]))
        dmat = raster.materials_device(mats)
        out = {k: vw.out(f16z(H, W), k) for k in ("albedo", "emissive", "normal", "velocity")}
        out["depth"] = vw.out(torch.zeros(H, W, dtype=torch.float32, device=DEV), "depth")
        vw.freeze()
        raster.gbuffer_resolve(g, dm, dmat, len(mats), vis, out["depth"], out["albedo"], out["emissive"], out["normal"],
                               out["velocity"], ws)
        torch.cuda.synchronize()
        for t, snap in keep:
            assert torch.equal(t.buf, snap)
        return out
    tight = run_layout(run, layout)

    def against_oracle():
        def host_tex(a, srgb):
            if not mipmapped:
                return a
            buf = np.zeros(raster.MipTexture.chain_bytes(32, 32), np.uint8)
            buf[:32 * 32 * 4] = a.reshape(-1)
            t = raster.MipTexture(buf, 32, 32, srgb)
            oracle.generate_mips(t)
            return t
        # a material holds addresses only: the host textures stay alive in these lists
        ha = [host_tex(tex[i], True) for i in range(len(tex))]
        hn = [host_tex(nrm[i], False) if mipmapped else None for i in range(len(tex))]
        hmats = [raster.material(albedo=ha[i], normal_texture=hn[i], **kw[i]) for i in range(len(tex))]
        vis_ref = np.zeros((H, W), np.uint64)
        oracle.raster_visibility(hm, vp, raster.CULL_FRONT, vis_ref)
        assert np.array_equal(host(vis).view(np.uint64), vis_ref)
        ref = {k: np.zeros((H, W, 4), np.float16) for k in ("albedo", "emissive", "normal", "velocity")}
        ref["depth"] = np.zeros((H, W), np.float32)
        oracle.gbuffer_resolve(g, hm, hmats, vis_ref, ref["depth"], ref["albedo"], ref["emissive"], ref["normal"],
                               ref["velocity"])
        assert np.array_equal(host(tight["depth"]), ref["depth"])
        for k in ("albedo", "emissive", "normal", "velocity"):
            assert f16_close(host(tight[k]), ref[k]).all(), k
    once(("gbuffer", mipmapped), against_oracle)


# ------------------------------------------------------------------------------------------------ terrain, Hi-Z
@pytest.mark.parametrize("layout", LAYOUTS)
def test_height_to_normal_and_terrain_tessellate(soc, oracle, layout):
    """64x64 heightmap view: the normal map (tight against the oracle here, bit-exact as test_height_to_normal_bit_exact)
    and the tessellated mesh (positions, normals, uvs, indices; tight bit-exact against the oracle as
    test_terrain_tessellate_bit_exact, grid 17 level 5)."""
    S, grid, level = 64, 17, 5
    g = globals_for(320, 180, camera=((20.0, 34.0, 20.0), (0.785, 0.6, 0.0)))
    h8 = scene.terrain_heightmap(S)

    def run(vw):
        hm = vw.inp(dev(h8), "heightmap")
        n = vw.out(f16z(S, S), "normal_target")
        vw.freeze()
        raster.height_to_normal(hm, n)
        m = raster.terrain_tessellate(g, hm, grid, level)
        return {"normal": n, "positions": m.positions, "normals": m.normals, "uvs": m.uvs, "indices": m.indices}
    tight = run_layout(run, layout)

    def against_oracle():
        ref = np.zeros(h8.shape, np.float16)
        oracle.height_to_normal(h8, ref)
        assert np.array_equal(host(tight["normal"]).view(np.uint16), ref.view(np.uint16))
        V, T = raster.terrain_tess_counts(grid, level)
        r = oracle.terrain_tessellate(g, h8, grid, level, V, T)
        for k in ("positions", "normals", "uvs"):
            assert np.array_equal(host(tight[k]).view(np.uint32), r[k].view(np.uint32)), k
        assert np.array_equal(host(tight["indices"]).view(np.uint32), r["indices"])
    once(("terrain",), against_oracle)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("op_max", [False, True])
@pytest.mark.parametrize("W,H", [(128, 72), (200, 120)])
def test_generate_hiz(soc, oracle, W, H, op_max, layout):
    """Every mip a view with its own index; the tight run against the oracle here (bit-exact, as test_hiz_bit_exact)."""
    from test_hiz import depth_field
    g = globals_for(W, H, frames=1)
    d = depth_field(W, H, W)
    n = raster.hiz_mip_count(W, H)
    shapes = [(max(1, (H // 2) >> i), max(1, (W // 2) >> i)) for i in range(n)]

    def run(vw):
        depth = vw.inp(dev(d), "depth")
        mips = [vw.out(torch.full(s, -7.0, dtype=torch.float32, device=DEV), f"mip{i}") for i, s in enumerate(shapes)]
        vw.freeze()
        raster.generate_hiz(g, depth, mips, op_max)
        return {f"mip{i}": m for i, m in enumerate(mips)}
    tight = run_layout(run, layout)

    def against_oracle():
        ref = [np.full(s, -7.0, np.float32) for s in shapes]
        oracle.generate_hiz(g, d, ref, op_max)
        for i, r in enumerate(ref):
            assert np.array_equal(host(tight[f"mip{i}"]), r), i
    once(("hiz", W, H, op_max), against_oracle)


# ------------------------------------------------------------------------------------------------ render graph
# The frame's images in index order. The images behind an alignment gate of the frame's fast paths take the even
# indices, so that `mixed` (pad16 at even indices) keeps the frame on those paths with every pitch different, while the
# ungated images (odd indices) are misaligned; `odd` takes every gate's unaligned side.
GATED = ("albedo", "emissive", "normal", "depth", "velocity", "color", "output", "history_color[0]", "history_color[1]",
         "history_velocity[0]", "history_velocity[1]", "bloom_output")
UNGATED = ("shadow", "noise", "ssao", "ssao_blur", "clouds", "bloom_mips[0]", "bloom_mips[1]", "bloom_mips[2]",
           "bloom_mips[3]")
FRAME_INDEX = dict({k: 2 * i for i, k in enumerate(GATED)}, **{k: 2 * i + 1 for i, k in enumerate(UNGATED)})


def _view_frame(soc, W, H, vw, shadow_size, **kw):
    """soc.alloc_frame with every image replaced by a view of `vw` holding the same contents. All of them are checked
    as outputs (padding intact): which of them a frame writes depends on the graph. The ones no pass of the graph
    writes are compared after the frames by the caller."""
    fr = soc.alloc_frame(W, H, DEV, **kw)
    fr["shadow"] = torch.ones(shadow_size, shadow_size, dtype=torch.float32, device=DEV)
    for k, index in FRAME_INDEX.items():
        name, _, i = k.partition("[")
        if i:
            fr[name][int(i[0])] = vw.inout(fr[name][int(i[0])], k, index)
        elif fr.get(name) is not None:
            fr[name] = vw.inout(fr[name], k, index)
    return fr


def _frame_results(fr, r):
    res = {k: fr[k].clone() for k in ("output", "color", "auto_exposure", "ssao", "ssao_blur", "clouds", "emissive")}
    res["resolved"] = r.resolved().clone()
    res["velocity_history"] = fr["history_velocity"][r.current_history()].clone()
    for i, m in enumerate(fr["bloom_mips"]):
        res[f"bloom_mip{i}"] = m.clone()
    if fr.get("bloom_output") is not None:
        res["bloom_output"] = fr["bloom_output"].clone()
    return res


# In `odd` the frame's TAA runs as taa_fast and a separate tone map instead of the pair kernel with the fused store.
# The two resolve the history with different lerp and Gaussian rounding orders (taa.hip: "Same per-pixel result as
# taa_fast within the RGBA16F tolerance"; no identity test claims their bits equal, and a few pixels of these frames
# differ in the last bit). For the resolved history and the framebuffer, (a) is therefore the passes' conditional oracle
# bound of helpers.frame_parity, asserted on every run by _taa_conditional: TAA from the run's own inputs within
# 1e-3 + 2e-3 |ref| on every value, the tone map of the run's own resolved history within 1 level, equal on >= 99.9 %.
TAA_FAST_RELAXED = ("resolved", "output")


def _taa_conditional(soc, oracle, g, fr, r, label):
    q = r.current_history()
    ref = np.zeros(tuple(fr["color"].shape), np.float16)
    oracle.temporal_antialiasing(g, ref, host(fr["color"]), host(fr["history_color"][1 - q]), host(fr["velocity"]),
                                 host(fr["history_velocity"][1 - q]), host(fr["depth"]))
    got = host(fr["history_color"][q])
    ok = f16_close(got, ref)
    assert ok.all(), (label, ok.mean(), np.argwhere(~ok)[:5])
    ae = soc.AutoExposure()
    ae.exposure = soc.exposure_of(fr["auto_exposure"])
    to = np.zeros(tuple(fr["output"].shape), np.uint8)
    oracle.tone_mapping(g, got, ae, to, fr.get("output_format"))
    d = np.abs(host(fr["output"]).astype(np.int32) - to.astype(np.int32))
    assert d.max() <= 1 and (d == 0).mean() >= 0.999, (label, d.max(), (d == 0).mean())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("flags", ["default", "sky_high_bloom_in_composition"])
def test_render_graph_frames(soc, oracle, flags, layout):
    """Two frames at 256x144 through a Renderer whose images are all views (own index each): framebuffer, colour,
    resolved history, exposure (and the intermediate images) equal those of the same frames on tight images, bit for
    bit (odd: TAA_FAST_RELAXED); padding intact on every canvas; the G-buffer, shadow and noise canvases unchanged.
    test_render_graph_frames (test_gpu_parity.py) checks the tight default frames against the oracle at this shape and
    these inputs."""
    W, H = 256, 144
    g, gb = sponza_inputs(W, H, elapsed=10.0)
    kw = {} if flags == "default" else dict(sky_lane_queue="high", bloom_in_composition=True)
    inputs = ("albedo", "normal", "velocity", "depth", "shadow", "noise")

    def run(vw):
        # the in-Composition bloom stage needs the separate bloom output; the default graph blooms the emissive in place
        fr = _view_frame(soc, W, H, vw, gb["shadow"].shape[0], bloom_output=flags != "default")
        for k in ("albedo", "emissive", "normal", "velocity", "depth", "shadow", "noise"):
            fr[k].copy_(torch.from_numpy(gb[k]))
        snaps = {k: c.clone() for k, _, c in vw.outs if k in inputs}
        r = soc.Renderer(fr, **kw)
        for f in range(2):
            fr["emissive"].copy_(torch.from_numpy(gb["emissive"]))   # the bloom chain overwrites it in place
            r.execute(g)
            _taa_conditional(soc, oracle, g, fr, r, (vw.layout, f))
        res = _frame_results(fr, r)
        r.close()
        for k, _, c in vw.outs:
            if k in inputs:
                assert bits_equal(c, snaps[k]), f"input canvas {k} changed"
        return res
    relaxed = TAA_FAST_RELAXED if layout == "odd" else ()
    if layout == "odd" and flags != "default":
        # composition_generic cannot compute the bloom stage, so the chain's fourth pass runs and writes the bloom
        # output, which the in-Composition stage of the tight frame leaves untouched
        # (test_bloom_in_composition_generic_resolution_frame): the colour image, compared bit for bit, holds its values
        relaxed += ("bloom_output",)
    run_layout(run, layout, relaxed=relaxed)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_render_graph_raster_head(soc, oracle, layout):
    """The raster head (DepthPrepass / SunShadowDraw / GBufferGeneration, shadow = 1) on the box atrium writing the
    G-buffer and the shadow map into views: two frames equal the tight frames bit for bit (odd: TAA_FAST_RELAXED),
    padding intact (SunShadowDraw clears the shadow view through soc_raster_depth's launcher).
    test_render_graph_raster_head (test_gpu_raster.py) ties the tight frames to the stand-alone calls."""
    W, H = 256, 144
    g = globals_for(W, H, camera=SPONZA_CAMERA, elapsed=10.0)
    sc = raster.scene_setup(g, scene.SPONZA_PROXY, tex_size=64)
    noise = scene.noise_texture()

    def run(vw):
        fr = _view_frame(soc, W, H, vw, 256, bloom_output=True)
        fr["noise"].copy_(torch.from_numpy(noise))
        fr["shadow"].zero_()
        vis = torch.zeros((H, W), dtype=torch.int64, device=DEV)
        r = soc.Renderer(fr)
        r.set_raster_scene(sc["mesh"], sc["materials"], sc["material_count"], vis, sc["workspace"], shadow=True)
        for f in range(2):
            r.execute(g)
            _taa_conditional(soc, oracle, g, fr, r, (vw.layout, f))
        res = _frame_results(fr, r)
        for k in ("depth", "albedo", "normal", "velocity", "shadow"):
            res[k] = fr[k].clone()
        r.close()
        return res
    tight = run_layout(run, layout, relaxed=TAA_FAST_RELAXED if layout == "odd" else ())
    assert (tight["depth"] < 1.0).float().mean() > 0.3 and (tight["shadow"] < 1.0).float().mean() > 0.001
