"""Composition's outputs against recorded bits (-m gpu): SHA-256 digests of the colour image, of the 256 histogram bins
where the call has them and of the shaded-pairs counter where it is given, compared with
tests/golden/composition_digests.json.

The digests were recorded once on an MI355X from a build of the commit BEFORE the launcher was split into
composition_plan.cpp's planner and composition.hip's issuer, never from the split itself: they hold a
refactor of the launcher, and of the kernels' shared device code, to the same bits. A change that is MEANT to move
Composition's arithmetic re-records the file from its own build, and says so:
    PYTHONPATH=.:oracle:tests python tests/test_gpu_composition_digests.py > tests/golden/composition_digests.json

Stand-alone entry points, at 64x36 (the pair path with a partial last tile row), 98x56 (partial tiles on both axes) and
97x55 (the generic kernels; a histogram call then runs the histogram pass): soc_composition and
soc_composition_luminance_histogram, their bounded twins with flags 0 and SOC_LIGHTS_CULL, with and without the counter
(light_bounds_scene's frame), and their cascaded twins (sun_cascades_scene's frame, the three-cascade record), each with
and without lights. The knob forms SOC_COMP_NT=0 and SOC_COMP_AOP=0 at 64x36 (without lights: the knobs reach no other
form). The renderer-only forms (sky_external, the in-kernel bloom, the zero cells as a flag and as a template argument)
through one renderer frame each at 192x64, forced as test_gpu_bloom_sparse.py forces them."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

import light_bounds_scene as lights_scene
import sun_cascades_scene as cascades_scene

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "composition_digests.json")
EXTENTS = [(64, 36), (98, 56), (97, 55)]
RENDERER_EXTENT = (192, 64)
# name -> keyword arguments of soc.composition / soc.composition_luminance_histogram
BOUNDED = {f"cull{int(cull)}_counter{int(counter)}": dict(cull=cull, counter=counter) for cull in (False, True) for counter in (False, True)}
KNOBS = {"nt0": {"SOC_COMP_NT": "0"}, "aop0": {"SOC_COMP_AOP": "0"}}
RENDERER_CASES = [f"renderer_{lane}_sparse{knob}_lights{int(lights)}" for lane in ("low", "high") for knob in "01" for lights in (False, True)]


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def without_lights(g):
    g = cascades_scene.copy_globals(g)
    g.point_light_count = g.spot_light_count = 0
    return g


class Rig:
    """The two frames' device inputs per extent, made once."""

    def __init__(self, soc):
        self.soc = soc
        self.frames = {}

    def frame(self, kind, W, H):
        if (kind, W, H) not in self.frames:
            soc = self.soc
            f = {}
            if kind == "lights":
                g, gb, ssao, clouds = lights_scene.frame_inputs(W, H)
                f["ins"] = [dev(a) for a in (gb["albedo"], gb["emissive"], gb["normal"], gb["depth"], ssao, gb["shadow"], clouds)]
                f["bounds"] = soc.light_bounds_device_buffer()
                soc.upload_light_bounds(soc.light_bounds(lights_scene.POINT_RANGES, lights_scene.SPOT_RANGES), f["bounds"])
            else:
                g0, gb, ssao, clouds = cascades_scene.frame_inputs(W, H)
                g = cascades_scene.set_lights(cascades_scene.copy_globals(g0))
                f["rec"] = cascades_scene.fit(g, *cascades_scene.RECORDS[0])
                f["ins"] = [dev(a) for a in cascades_scene.host_inputs(gb, ssao, clouds, cascades_scene.atlas(g, f["rec"]))]
            f["g"] = {True: g, False: without_lights(g)}
            f["dg"] = {}
            for lit, gl in f["g"].items():
                f["dg"][lit] = soc.globals_device_buffer()
                soc.upload_globals(gl, f["dg"][lit])
            self.frames[kind, W, H] = f
        return self.frames[kind, W, H]

    def run(self, kind, W, H, lit, fused, cull=None, counter=False):
        """{colour, bins, counter: digest} of one stand-alone call."""
        soc, f = self.soc, self.frame(kind, W, H)
        out = torch.zeros(H, W, 4, dtype=torch.float16, device=DEV)
        kw = dict(d_globals=f["dg"][lit])
        n = torch.zeros(1, dtype=torch.int32, device=DEV) if counter else None
        if cull is not None:
            kw.update(bounds=f["bounds"], cull=cull, shaded_pairs=n)
        if kind == "cascades":
            kw.update(cascades=f["rec"])
        res = {}
        if fused:
            ae = soc.auto_exposure_buffer()
            soc.composition_luminance_histogram(f["g"][lit], out, *f["ins"], ae, soc.histogram_scratch(), **kw)
            bins = ae.view(torch.int32)[1:]
            torch.cuda.synchronize()
            assert int(bins.sum()) == W * H
            res["bins"] = sha(bins)
        else:
            soc.composition(f["g"][lit], out, *f["ins"], **kw)
        res["colour"] = sha(out.view(torch.int16))
        if counter:
            res["counter"] = sha(n)
        return res


def standalone_cases():
    """name -> arguments of Rig.run"""
    cases = {}
    for W, H in EXTENTS:
        for lit in (False, True):
            for fused in (False, True):
                tag = f"{W}x{H}_lights{int(lit)}_{'histogram' if fused else 'plain'}"
                cases[f"composition_{tag}"] = ("lights", W, H, lit, fused)
                cases[f"cascaded_{tag}"] = ("cascades", W, H, lit, fused)
                for name, kw in BOUNDED.items():
                    cases[f"bounded_{name}_{tag}"] = ("lights", W, H, lit, fused, kw["cull"], kw["counter"])
    return cases


STANDALONE = standalone_cases()


def knob_case(soc, rig, setenv, delenv, knob, fused):
    for k, v in KNOBS[knob].items():
        setenv(k, v)
    soc.reload_tuning()
    res = rig.run("lights", 64, 36, False, fused)
    for k in KNOBS[knob]:
        delenv(k)
    soc.reload_tuning()
    return res


def renderer_case(soc, patch, name):
    """One renderer frame with the in-kernel bloom allowed, executed as PRE_EXPOSURE then POST_EXPOSURE so that the 256
    bins can be read between the two (LuminanceHistogramFold has added the partials; AutoExposure, which zeroes them, has
    not run). lane low: the zero cells beside the chain's last stage (sparse 1) or the dense frame (0); lane high: the
    in-kernel bloom, with the cells' proof (1) or without. All under the sky split (sky_external, SkyCompose's bins). The
    emissive image is zero but for one lit texel, so most cells are proven. Which form ran is asserted from the bloom
    output: untouched (in-kernel bloom), untouched in the proven cells only (zero cells), or written everywhere.
    -> {colour, bins (the 256 bins), and after the whole frame: exposure (the AutoExposure block), output (tone-mapped)}"""
    import ctypes as C

    import test_gpu_bloom_sparse as bs
    _, lane, sparse, lights = name.split("_")
    W, H = RENDERER_EXTENT
    patch.setenv("SOC_BLOOM_SPARSE", sparse[-1])
    soc.reload_tuning()
    g0, gb = bs.inputs(W, H)
    fr = soc.alloc_frame(W, H, DEV, bloom_output=True)
    for k in ("albedo", "normal", "velocity", "depth"):
        fr[k].copy_(torch.from_numpy(gb[k]))
    fr["emissive"].copy_(torch.from_numpy(bs.lit_u16(H, W, 40, 20).view(np.float16)))
    fr["shadow"] = dev(gb["shadow"])
    fr["noise"].copy_(torch.from_numpy(gb["noise"]))
    fr["bloom_output"].fill_(bs.SENTINEL)
    r = soc.Renderer(fr, bloom_in_composition=True, sky_lane_queue=lane)
    assert "SkyCompose" in r.pass_names()
    g = type(g0)()
    C.pointer(g)[0] = g0
    if lights[-1] == "1":
        import bench
        soc.scene_update(g, bench.point_lights_c3b())
    r.execute(g, soc.PHASE_PRE_EXPOSURE)
    torch.cuda.synchronize()
    bins = fr["auto_exposure"].view(torch.int32)[1:].clone()
    res = {"colour": sha(fr["color"].view(torch.int16)), "bins": sha(bins)}
    untouched = bs.sentinel_mask(fr["bloom_output"])
    r.execute(g, soc.PHASE_POST_EXPOSURE)
    res["exposure"] = sha(fr["auto_exposure"].view(torch.int32))
    res["output"] = sha(fr["output"])
    r.close()
    patch.delenv("SOC_BLOOM_SPARSE")
    soc.reload_tuning()
    assert int(bins.sum()) == W * H, int(bins.sum())
    if lane == "high":
        assert untouched.all()
    elif sparse[-1] == "1":
        assert untouched.any() and not untouched.all()
    else:
        assert not untouched.any()
    return res


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN_PATH) as f:
        return json.load(f)["digests"]


@pytest.fixture(scope="module")
def rig(soc):
    return Rig(soc)


def test_fixture_covers_the_cases(golden):
    names = list(STANDALONE) + [f"knob_{k}_{f}" for k in KNOBS for f in ("plain", "histogram")] + RENDERER_CASES
    assert sorted(golden) == sorted(names)


@pytest.mark.parametrize("name", sorted(STANDALONE))
def test_standalone_digest(rig, golden, name):
    assert rig.run(*STANDALONE[name]) == golden[name]


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("knob", sorted(KNOBS))
def test_knob_form_digest(soc, rig, monkeypatch, golden, knob, fused):
    got = knob_case(soc, rig, monkeypatch.setenv, monkeypatch.delenv, knob, fused)
    assert got == golden[f"knob_{knob}_{'histogram' if fused else 'plain'}"]


@pytest.mark.parametrize("name", RENDERER_CASES)
def test_renderer_form_digest(soc, monkeypatch, golden, name):
    assert renderer_case(soc, monkeypatch, name) == golden[name]


class _Env:
    """monkeypatch's two methods on os.environ, for record()"""
    setenv = staticmethod(os.environ.__setitem__)
    delenv = staticmethod(os.environ.__delitem__)


def record():
    """Every digest of this file as the JSON document the tests read (run on an MI355X; see the module docstring)."""
    import soc_real_time_renderer_amd as soc
    soc.lib()
    rig = Rig(soc)
    digests = {name: rig.run(*args) for name, args in STANDALONE.items()}
    for knob in KNOBS:
        for fused in (False, True):
            digests[f"knob_{knob}_{'histogram' if fused else 'plain'}"] = knob_case(soc, rig, _Env.setenv, _Env.delenv, knob, fused)
    for name in RENDERER_CASES:
        digests[name] = renderer_case(soc, _Env, name)
    doc = {"comment": "SHA-256 of Composition's colour image, histogram bins and shaded-pairs counter "
                      "(tests/test_gpu_composition_digests.py), recorded on an MI355X from the commit before the launcher was split "
                      "into a planner and an issuer. An intended change of Composition's arithmetic re-records this file (see that "
                      "module's docstring); nothing else does.",
           "digests": digests}
    json.dump(doc, sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")


if __name__ == "__main__":
    record()
