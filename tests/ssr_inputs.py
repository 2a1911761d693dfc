"""Inputs of the ScreenSpaceReflection tests, shared by the CPU sensitivity check (test_ssr_oracle.py) and the GPU
parity check (test_gpu_ssr.py), with the float32 oracle's result for each, computed once per session."""
import numpy as np

import helpers
import ssr_oracle

# name -> (builder, arguments): the synthesised Sponza atrium at an odd extent that is a multiple of no tile and at
# 96x54, the orthographic and oblique projections (a constant and a position-dependent w row of the inverse projection),
# and the terrain (half sky, two thirds of the rays miss)
INPUTS = {
    "sponza_67x41": ("variant", "default", 67, 41),
    "sponza_96x54": ("variant", "default", 96, 54),
    "ortho_96x54": ("variant", "ssao_ortho", 96, 54),
    "oblique_96x54": ("variant", "ssao_oblique", 96, 54),
    "terrain_160x90": ("terrain", None, 160, 90),
}

_CACHE = {}
_REFERENCE = {}


def inputs(name):
    """(globals, G-buffer dict, metallic-roughness RGBA16F) of the named input; the arrays are shared: do not write."""
    if name not in _CACHE:
        kind, variant, W, H = INPUTS[name]
        if kind == "variant":
            g, gb = helpers.cached_variant_inputs(variant, W, H)
        else:
            g, gb = helpers.terrain_inputs(W, H)
        _CACHE[name] = (g, gb, ssr_oracle.metallic_roughness_pattern(H, W))
    return _CACHE[name]


def run_oracle(name, dtype):
    g, gb, mr = inputs(name)
    return ssr_oracle.screen_space_reflection(g, gb["depth"], gb["normal"], gb["albedo"], mr, dtype)


def reference(name):
    """The float32 oracle's (rgba float16, steps uint8) of the named input: the yardstick."""
    if name not in _REFERENCE:
        _REFERENCE[name] = run_oracle(name, np.float32)
    return _REFERENCE[name]


def disagreeing(rgba, steps, ref_rgba, ref_steps):
    """Per-pixel mask: the step counts differ, or a colour channel is outside helpers.f16_close of the reference's."""
    return (steps != ref_steps) | ~helpers.f16_close(rgba, ref_rgba).all(axis=-1)
