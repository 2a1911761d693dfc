"""cascades_oracle — Composition with cascaded sun shadow maps in numpy (TEST INFRASTRUCTURE; soc_composition_cascaded,
DESIGN.md §5.8).

np_oracle.composition (oracle/np_oracle.py, written from composition.inl:110-225) with the sun's one map replaced by the
cascades of a soc_sun_cascades record, built on that module's helpers (centres, bilinear, mat, apply, normalize, vec,
unorm8), which are imported, not copied:

* a pixel uses cascade k = the number of i < count - 1 with depth > split_depth[i], compared as float32 values (a NaN
  depth compares false: cascade 0);
* the shadow term is the reference's (composition.inl:166-173) per cascade: project the world position with
  projection_view[k], one bilinear tap at xy * 0.5 + 0.5 inside slab k = atlas[k * S:(k + 1) * S] (so clamp-to-edge stays
  in the slab), clamp(pow(exp(exponential_factor[k] * (z - d)), darkening_factor), 0, 1); selected per pixel with
  np.where over the per-slab taps; no blending.

Everything is float64, as np_oracle. The cascades have no counterpart in the reference: this oracle and the one-cascade
identity (a record of the sun itself gives np_oracle.composition's bits) are what pins them.

Returns the RGBA16F image, the per-pixel cascade index (H, W) int and, per 16 x 8 patch (the pixels one wave of
composition_pair covers), PURE / MIXED / NONE: its lit pixels (depth != 1) select one cascade, several, or it has none.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "oracle") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
import np_oracle as npo  # noqa: E402
from np_oracle import apply, bilinear, centres, mat, normalize, unorm8, vec  # noqa: E402

PATCH_W, PATCH_H = 16, 8
NONE, PURE, MIXED = 0, 1, 2


def select(depth, record):
    """The cascade of every pixel of an (H, W) float32 depth image: a count of float32 compares."""
    d = np.asarray(depth, np.float32)
    k = np.zeros(d.shape, np.int64)
    with np.errstate(invalid="ignore"):
        for i in range(int(record.count) - 1):
            k += d > np.float32(record.split_depth[i])
    return k


def patch_kinds(k, lit):
    """(ceil(H / 8), ceil(W / 16)) array of NONE / PURE / MIXED over the lit pixels of each 16 x 8 patch."""
    H, W = k.shape
    ph, pw = -(-H // PATCH_H), -(-W // PATCH_W)
    kinds = np.zeros((ph, pw), np.int64)
    for py in range(ph):
        for px in range(pw):
            blk = (slice(py * PATCH_H, (py + 1) * PATCH_H), slice(px * PATCH_W, (px + 1) * PATCH_W))
            n = len(np.unique(k[blk][lit[blk]]))
            kinds[py, px] = NONE if n == 0 else PURE if n == 1 else MIXED
    return kinds


def composition(g, albedo, emissive, normal, depth, ssao, atlas, clouds, record, subtexel_bits=None):
    """-> (RGBA16F image, cascade index per pixel, kind per 16 x 8 patch). subtexel_bits: np_oracle.SUBTEXEL_BITS for this
    call (8: the filter weights of the sampling contract the kernels follow)."""
    old = npo.SUBTEXEL_BITS
    npo.SUBTEXEL_BITS = subtexel_bits
    try:
        return _composition(g, albedo, emissive, normal, depth, ssao, atlas, clouds, record)
    finally:
        npo.SUBTEXEL_BITS = old


def _composition(g, albedo, emissive, normal, depth, ssao, atlas, clouds, record):
    H, W = depth.shape
    count, S = int(record.count), int(record.map_size)
    assert atlas.shape == (count * S, S), (atlas.shape, count, S)
    u, v = centres(W, H)
    d = bilinear(depth, u, v)
    inv_proj, inv_view = mat(g.camera_inverse_projection_matrix), mat(g.camera_inverse_view_matrix)
    clip = np.stack([u * 2 - 1, v * 2 - 1, d, np.ones_like(d)], -1)
    vs = apply(inv_proj, clip)
    vs = vs / vs[..., 3:4]
    world = apply(inv_view, vs)[..., :3]
    k = select(d, record)
    world1 = np.concatenate([world, np.ones_like(d)[..., None]], -1)
    sun_shadow = np.zeros_like(d)
    for c in range(count):
        sp = apply(mat(record.projection_view[c]), world1)
        pc = sp[..., :3] / sp[..., 3:4]
        sd = bilinear(atlas[c * S:(c + 1) * S], pc[..., 0] * 0.5 + 0.5, pc[..., 1] * 0.5 + 0.5)
        with np.errstate(over="ignore", invalid="ignore"):
            term = np.clip(np.power(np.exp(float(record.exponential_factor[c]) * (pc[..., 2] - sd)),
                                    g.sun_info.darkening_factor), 0.0, 1.0)
        sun_shadow = np.where(k == c, term, sun_shadow)
    em = bilinear(emissive, u, v)[..., :3] * g.emissive_bloom_strength
    al = bilinear(albedo, u, v)[..., :3]
    nn = bilinear(normal, u, v)[..., :3]
    occ = np.power(bilinear(unorm8(ssao), u, v), g.ambient_occlussion_strength)
    sun_dir = vec(g.sun_info.direction)
    direct = (np.maximum(0.0, nn @ -sun_dir) * sun_shadow)[..., None] * np.ones(3)
    cam = vec(g.camera_position)
    view_dir = normalize(cam - world)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(int(g.point_light_count)):      # calculate_point_light, :124-139
            L = g.point_lights[i]
            lp = vec(L.position)
            ld = normalize(lp - world)
            dist = np.linalg.norm(lp - world, axis=-1)
            att = 1.0 / (dist * dist)
            hw = normalize(ld + view_dir)
            diffuse = np.maximum(np.sum(nn * ld, -1), 0.0)
            nh = np.arccos(np.clip(np.sum(hw * nn, -1), -1.0, 1.0))
            direct += al * vec(L.color) * ((diffuse + np.exp(-(nh * nh))) * att * L.intensity)[..., None]
        for i in range(int(g.spot_light_count)):       # calculate_spot_light, :141-160
            L = g.spot_lights[i]
            lp = vec(L.position)
            ld = normalize(lp - world)
            theta = ld @ (-vec(L.direction) / np.linalg.norm(vec(L.direction)))
            inten = np.clip((theta - L.outer_cut_off) / (L.cut_off - L.outer_cut_off), 0.0, 1.0)
            dist = np.linalg.norm(lp - world, axis=-1)
            att = 1.0 / (dist * dist)
            hw = normalize(ld + view_dir)
            diffuse = np.maximum(np.sum(nn * ld, -1), 0.0)
            nh = np.arccos(np.clip(np.sum(hw * nn, -1), -1.0, 1.0))
            direct += al * vec(L.color) * ((diffuse + np.exp(-(nh * nh))) * att * L.intensity * inten)[..., None]
    color = (direct + vec(g.ambient)) * al * occ[..., None] + em
    sky = d == 1.0
    color[sky] = bilinear(unorm8(clouds), u, v)[..., :3][sky]
    out = np.concatenate([color, np.ones_like(d)[..., None]], -1)
    return out.astype(np.float16), k, patch_kinds(k, ~sky)
