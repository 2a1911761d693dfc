"""Inputs of the depth-of-field tests, shared by the CPU checks (test_dof_oracle.py) and the GPU parity checks
(test_gpu_dof.py), with the float32 oracle's chain and results for each, computed once per session.

Sizes: 64x36 (even extents, four 16x16 tiles across), 97x55 (odd, a multiple of no tile) and 33x17 (odd, a level of one
row early in the chain). Colour: random RGBA16F in [0, 4) with a twentieth of the texels zero and a few values near the
float16 maximum; alpha random, not 1. Depth: d = (far - far near / od) / (far - near) of an object distance od log-spaced
from 0.2 to 990 along x with +-10 % jitter per pixel (the far end's jitter passes the far plane: those pixels have
depth >= 1 and are copied like the sky); the top max(2, H / 8) rows are the sky, 1.0. Two globals sets: the renderer's
defaults (plane_in_focus = 1) and plane_in_focus = 20, aperture = 2.8, focal_length = 0.05."""
import numpy as np

import dof_oracle
import helpers

SIZES = [(64, 36), (97, 55), (33, 17)]
GLOBALS = ["defaults", "focus20"]

_CACHE = {}


def globals_set(name, W, H):
    g = helpers.globals_for(W, H)
    if name == "focus20":
        g.plane_in_focus, g.aperture, g.focal_length = 20.0, 2.8, 0.05
    else:
        assert name == "defaults" and g.plane_in_focus == 1.0
    return g


def depth_from_distance(g, od):
    """The D32F depth of an object distance (the inverse of the shader's line 180), float64 rounded once."""
    near, far = float(g.camera_near_clip), float(g.camera_far_clip)
    return ((far - far * near / np.asarray(od, np.float64)) / (far - near)).astype(np.float32)


def images(W, H):
    """(color float16 (H, W, 4), depth float32 (H, W)); shared: do not write."""
    key = ("images", W, H)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 * W + H)
        color = rng.uniform(0.0, 4.0, (H, W, 4)).astype(np.float32)
        color[rng.uniform(size=(H, W)) < 0.05] = 0.0
        hot = rng.uniform(size=(H, W, 4)) < 0.004
        color[hot] = rng.uniform(60000.0, 65504.0, int(hot.sum()))
        color[..., 3] = rng.uniform(0.0, 0.9, (H, W))
        od = np.geomspace(0.2, 990.0, W)[None, :] * rng.uniform(0.9, 1.1, (H, W))
        depth = depth_from_distance(helpers.globals_for(W, H), od)
        depth[:max(2, H // 8)] = 1.0
        _CACHE[key] = (color.astype(np.float16), depth)
    return _CACHE[key]


def levels(W, H):
    """The float32 oracle's chain of images(W, H)'s colour."""
    key = ("levels", W, H)
    if key not in _CACHE:
        _CACHE[key] = dof_oracle.chain(images(W, H)[0])
    return _CACHE[key]


def reference(W, H, gname, dtype=np.float32, lq_offset=0):
    """(rgba float16, lq int32) of dof_oracle.depth_of_field on the inputs; the float32 runs are the yardstick."""
    key = ("ref", W, H, gname, np.dtype(dtype).name, lq_offset)
    if key not in _CACHE:
        _CACHE[key] = dof_oracle.depth_of_field(globals_set(gname, W, H), images(W, H)[1], levels(W, H), dtype, lq_offset)
    return _CACHE[key]


def check_against_oracle(rgba, W, H, gname, depth=None, level_list=None, g=None):
    """The parity rule: every pixel of `rgba` (float16 (H, W, 4)) equals, bit for bit, the float32 oracle's pixel at
    lq_offset -1, 0 or +1. Returns the share of geometry pixels that do not equal lq_offset 0. With depth / level_list / g
    the oracle runs on those instead of the cached inputs."""
    if depth is None:
        refs = [reference(W, H, gname, np.float32, o)[0] for o in (0, -1, 1)]
        depth = images(W, H)[1]
    else:
        refs = [dof_oracle.depth_of_field(g, depth, level_list, np.float32, o)[0] for o in (0, -1, 1)]
    got = np.ascontiguousarray(rgba).view(np.uint16)
    same = [(got == r.view(np.uint16)).all(axis=-1) for r in refs]
    anyof = same[0] | same[1] | same[2]
    assert anyof.all(), (f"{int((~anyof).sum())} pixels equal the oracle at no lq_offset; first (y, x): "
                         f"{np.argwhere(~anyof)[:5].tolist()}")
    with np.errstate(invalid="ignore"):
        geom = depth < np.float32(1.0)
    sky_ok = same[0][~geom].all()
    assert sky_ok, "a copied pixel is not a bit copy of the level-0 texel"
    return float((~same[0][geom]).mean()) if geom.any() else 0.0
