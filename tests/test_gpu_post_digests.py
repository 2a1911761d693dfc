"""The TAA, SSAO and bloom passes' outputs against recorded bits (-m gpu): SHA-256 digests of every output image,
compared with tests/golden/post_digests.json.

The digests were recorded once on an MI355X from a build of the commit BEFORE these passes' launchers were split into
post_plan.cpp's planners and the issuers in taa.hip, ssao.hip, bloom_w.hip and bloom.hip, never from
the split itself: they hold a refactor of the launchers to the same bits. A change that is MEANT to move one of these
passes' arithmetic re-records the file from its own build, and says so:
    PYTHONPATH=.:oracle:tests python tests/test_gpu_post_digests.py > tests/golden/post_digests.json

TAA (both entry points: target, velocity_history_out, the RGBA8 output) at 64x36, 130x58 (two tile columns, rows not a
multiple of 4), 97x55 (taa_fast) and with the colour image at half extent (taa_generic); SOC_TAA_NBR 0..3 and a depth
image whose base is 8 bytes off (taa_pair2) at 64x36. SSAO generation and blur for frames of 128x72, 260x130 and 97x55,
with and without the noise table; SOC_SSAO_TILE=0 and SOC_SSAO_PIPE 0 and 2 at 128x72. The weighted bloom chain's mip 1,
mip 3 and output at 64x48 and 200x104, as stage 0 and as stages 1-4; the per-pass chain at 64x48 and at 97x55, where the
mips do not halve. One renderer frame at 192x64 with the sparse bloom output forced as test_gpu_bloom_sparse.py forces
it: the proven-zero strips are never written, so the bloom output is pre-filled with that module's sentinel."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from helpers import random_rgba16, sponza_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "post_digests.json")
TAA_KNOBS = {f"nbr{n}": {"SOC_TAA_NBR": str(n)} for n in range(4)}
SSAO_KNOBS = {"tile0": {"SOC_SSAO_TILE": "0"}, "pipe0": {"SOC_SSAO_PIPE": "0"}, "pipe2": {"SOC_SSAO_PIPE": "2"}}
TAA_CASES = {"64x36": (64, 36, {}), "130x58": (130, 58, {}), "97x55": (97, 55, {}), "half_colour": (64, 36, dict(half_colour=True)),
             "depth_off8": (64, 36, dict(depth_off8=True)), **{k: (64, 36, dict(env=e)) for k, e in TAA_KNOBS.items()}}
SSAO_CASES = {**{f"{w}x{h}_table{int(t)}": (w, h, t, {}) for w, h in ((128, 72), (260, 130), (97, 55)) for t in (True, False)},
              **{k: (128, 72, True, e) for k, e in SSAO_KNOBS.items()}}
BLOOM_W_EXTENTS = [(64, 48), (200, 104)]
BLOOM_CHAIN_EXTENTS = [(64, 48), (97, 55)]
_INPUTS = {}


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def inputs(W, H):
    """The frame's globals and host G-buffer, made once per extent and left unchanged."""
    if (W, H) not in _INPUTS:
        _INPUTS[W, H] = sponza_inputs(W, H)
    return _INPUTS[W, H]


class Env:
    """Knobs for the length of one case; patch has monkeypatch's setenv / delenv."""

    def __init__(self, soc, patch, env):
        self.soc, self.patch, self.env = soc, patch, env

    def __enter__(self):
        for k, v in self.env.items():
            self.patch.setenv(k, v)
        self.soc.reload_tuning()

    def __exit__(self, *exc):
        for k in self.env:
            self.patch.delenv(k)
        self.soc.reload_tuning()


def taa_case(soc, patch, name):
    W, H, opt = TAA_CASES[name]
    g, gb = inputs(W, H)
    cw, ch = (W // 2, H // 2) if opt.get("half_colour") else (W, H)
    colour, history = dev(random_rgba16(ch, cw, 1)), dev(random_rgba16(H, W, 2))
    vel, pvel = dev(gb["velocity"]), dev(random_rgba16(H, W, 3, lo=-0.01, hi=0.01))
    if opt.get("depth_off8"):
        flat = torch.zeros(H * W + 2, dtype=torch.float32, device=DEV)
        depth = flat[2:].view(H, W)
        depth.copy_(torch.from_numpy(gb["depth"]))
        assert depth.data_ptr() % 16 == 8
    else:
        depth = dev(gb["depth"])
    ae = soc.auto_exposure_buffer(DEV, exposure=0.8)
    res = {}
    with Env(soc, patch, opt.get("env", {})):
        for entry in ("plain", "tone_mapping"):
            target, vho = torch.zeros(H, W, 4, dtype=torch.float16, device=DEV), torch.zeros(H, W, 4, dtype=torch.float16, device=DEV)
            if entry == "plain":
                soc.temporal_antialiasing(g, target, colour, history, vel, pvel, depth, velocity_history_out=vho)
            else:
                out = torch.zeros(H, W, 4, dtype=torch.uint8, device=DEV)
                soc.temporal_antialiasing_tone_mapping(g, target, colour, history, vel, pvel, depth, ae, out, velocity_history_out=vho)
                res[f"{entry}_output"] = sha(out)
            res[f"{entry}_target"] = sha(target.view(torch.int16))
            res[f"{entry}_velocity_history_out"] = sha(vho.view(torch.int16))
    return res


def ssao_case(soc, patch, name):
    W, H, table, env = SSAO_CASES[name]
    g, gb = inputs(W, H)
    depth, normal = dev(gb["depth"]), dev(gb["normal"])
    ao, blur = (torch.zeros(H // 2, W // 2, dtype=torch.uint8, device=DEV) for _ in range(2))
    noise = None
    if table:
        noise = torch.zeros((H // 2) * (W // 2) * 2, dtype=torch.float32, device=DEV)
        soc.ssao_prepare_noise(normal, ao, noise)
    with Env(soc, patch, env):
        soc.ssao_generation(g, depth, normal, ao, noise)
        soc.ssao_blur(g, ao, blur)
    res = {"ssao": sha(ao), "blur": sha(blur)}
    if table:
        res["noise_table"] = sha(noise.view(torch.int32))
    return res


def mips_of(W, H):
    return [torch.zeros(max(H >> i, 1), max(W >> i, 1), 4, dtype=torch.float16, device=DEV) for i in range(4)]


def bloom_weighted_case(soc, W, H, staged):
    g, _ = inputs(W, H)
    emissive, mips, out = dev(random_rgba16(H, W, 4, hi=2.0)), mips_of(W, H), torch.zeros(H, W, 4, dtype=torch.float16, device=DEV)
    for stage in ((1, 2, 3, 4) if staged else (0,)):
        soc.bloom_weighted_stage(g, emissive, mips, out, stage)
    return {"mip1": sha(mips[1].view(torch.int16)), "mip3": sha(mips[3].view(torch.int16)), "output": sha(out.view(torch.int16))}


def bloom_chain_case(soc, W, H):
    g, _ = inputs(W, H)
    emissive, mips = dev(random_rgba16(H, W, 5, hi=2.0)), mips_of(W, H)
    soc.bloom_chain(g, emissive, mips)
    return {"emissive": sha(emissive.view(torch.int16)), **{f"mip{i}": sha(m.view(torch.int16)) for i, m in enumerate(mips)}}


def renderer_case(soc, patch):
    """One frame whose emissive image is zero but for one lit texel, the zero cells beside the chain's last stage."""
    import ctypes as C

    import test_gpu_bloom_sparse as bs
    W, H = 192, 64
    with Env(soc, patch, {"SOC_BLOOM_SPARSE": "1"}):
        g0, gb = bs.inputs(W, H)
        fr = soc.alloc_frame(W, H, DEV, bloom_output=True)
        for k in ("albedo", "normal", "velocity", "depth"):
            fr[k].copy_(torch.from_numpy(gb[k]))
        fr["emissive"].copy_(torch.from_numpy(bs.lit_u16(H, W, 40, 20).view(np.float16)))
        fr["shadow"] = dev(gb["shadow"])
        fr["noise"].copy_(torch.from_numpy(gb["noise"]))
        fr["bloom_output"].fill_(bs.SENTINEL)   # the same fixed value on every run: the proven-zero strips keep it
        r = soc.Renderer(fr, bloom_in_composition=True, sky_lane_queue="low")
        g = type(g0)()
        C.pointer(g)[0] = g0
        r.execute(g)
        torch.cuda.synchronize()
        untouched = bs.sentinel_mask(fr["bloom_output"])
        res = {"bloom_output": sha(fr["bloom_output"].view(torch.int16)), "mip1": sha(fr["bloom_mips"][1].view(torch.int16)),
               "mip3": sha(fr["bloom_mips"][3].view(torch.int16)), "ssao": sha(fr["ssao"]), "ssao_blur": sha(fr["ssao_blur"]),
               "colour": sha(fr["color"].view(torch.int16)), "history": sha(fr["history_color"][0].view(torch.int16)),
               "history_velocity": sha(fr["history_velocity"][0].view(torch.int16)), "output": sha(fr["output"])}
        r.close()
    assert untouched.any() and not untouched.all()   # the sparse last stage ran
    return res


def all_cases(soc, patch):
    """name -> a function returning the case's digests"""
    cases = {f"taa_{n}": (lambda n=n: taa_case(soc, patch, n)) for n in TAA_CASES}
    cases.update({f"ssao_{n}": (lambda n=n: ssao_case(soc, patch, n)) for n in SSAO_CASES})
    for W, H in BLOOM_W_EXTENTS:
        for staged in (False, True):
            cases[f"bloom_weighted_{W}x{H}_{'stages' if staged else 'chain'}"] = lambda W=W, H=H, s=staged: bloom_weighted_case(soc, W, H, s)
    for W, H in BLOOM_CHAIN_EXTENTS:
        cases[f"bloom_chain_{W}x{H}"] = lambda W=W, H=H: bloom_chain_case(soc, W, H)
    cases["renderer_sparse_bloom"] = lambda: renderer_case(soc, patch)
    return cases


NAMES = sorted(all_cases(None, None))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN_PATH) as f:
        return json.load(f)["digests"]


def test_fixture_covers_the_cases(golden):
    assert sorted(golden) == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_digest(soc, monkeypatch, golden, name):
    assert all_cases(soc, monkeypatch)[name]() == golden[name]


def test_staged_chain_is_the_chain(golden):
    """The fixture itself: stages 1-4 one by one leave what stage 0 leaves."""
    for W, H in BLOOM_W_EXTENTS:
        assert golden[f"bloom_weighted_{W}x{H}_stages"] == golden[f"bloom_weighted_{W}x{H}_chain"]


class _Env:
    """monkeypatch's two methods on os.environ, for record()"""
    setenv = staticmethod(os.environ.__setitem__)
    delenv = staticmethod(os.environ.__delitem__)


def record():
    """Every digest of this file as the JSON document the tests read (run on an MI355X; see the module docstring)."""
    import soc_real_time_renderer_amd as soc
    soc.lib()
    digests = {name: case() for name, case in all_cases(soc, _Env).items()}
    doc = {"comment": "SHA-256 of the TAA, SSAO and bloom passes' output images (tests/test_gpu_post_digests.py), recorded on an "
                      "MI355X from the commit before their launchers were split into planners and issuers. An intended change of "
                      "one of these passes' arithmetic re-records this file (see that module's docstring); nothing else does.",
           "digests": digests}
    json.dump(doc, sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")


if __name__ == "__main__":
    record()
