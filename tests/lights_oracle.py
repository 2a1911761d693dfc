"""lights_oracle — Composition with bounded lights in numpy (TEST INFRASTRUCTURE; soc_composition_bounded).

np_oracle.composition (oracle/np_oracle.py, written from composition.inl:110-225) with the bounded semantics added, built
on that module's helpers (centres, bilinear, mat, apply, normalize), which are imported, not copied:

* a light with a range r > 0 is multiplied by the window w = clamp(1 - (d^2 / r^2)^2, 0, 1); r = 0 is unlimited: no
  window, not even a multiply by 1;
* f = w for a point light, f = w * cone term for a spot light (the cone term alone when unlimited); a light is added to
  a pixel only where f > 0 (a select: elsewhere the pixel keeps its bits, whatever the light's term is); an unlimited
  point light is added as np_oracle adds it, so a call without spot lights and with all ranges 0 gives np_oracle's bits.

dtype = float64 (np_oracle's precision) or float32 (the light loops in the device's precision; the sampling and the
matrix products stay np_oracle's float64 helpers, rounded to float32 where the loops start).

`reach[py, px, k]`: whether light k (point lights first, then spot lights) has f > 0 on any lit pixel (depth != 1) of
the 16 x 8 patch (px, py) one wave of composition_pair covers; `lit[py, px]`: the patch has a lit pixel.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "oracle") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
import np_oracle as npo  # noqa: E402
from np_oracle import apply, bilinear, centres, mat, normalize  # noqa: E402

PATCH_W, PATCH_H = 16, 8


def _vec(v, dt):
    return np.array(list(v), dt)


def window(d2, r, dt=np.float64):
    """KHR_lights_punctual's window on the squared distance: clamp(1 - (d^2 / r^2)^2, 0, 1)."""
    q = d2 / dt(dt(r) * dt(r))
    return np.fmin(np.fmax(dt(1.0) - q * q, dt(0.0)), dt(1.0))


def composition(g, albedo, emissive, normal, depth, ssao, shadow, clouds, point_ranges=(), spot_ranges=(),
                dtype=np.float64, subtexel_bits=None, linear=False):
    """-> (RGBA16F image, reach, lit). subtexel_bits: np_oracle.SUBTEXEL_BITS for this call (8: the filter weights of
    the sampling contract the kernels follow). linear: the (H, W, 3) colour before the RGBA16F store instead of the image."""
    old = npo.SUBTEXEL_BITS
    npo.SUBTEXEL_BITS = subtexel_bits
    try:
        return _composition(g, albedo, emissive, normal, depth, ssao, shadow, clouds, list(point_ranges), list(spot_ranges),
                            dtype, linear)
    finally:
        npo.SUBTEXEL_BITS = old


def _composition(g, albedo, emissive, normal, depth, ssao, shadow, clouds, point_ranges, spot_ranges, dt, linear):
    H, W = depth.shape
    npl, nsl = int(g.point_light_count), int(g.spot_light_count)
    pr = point_ranges + [0.0] * (npl - len(point_ranges))
    sr = spot_ranges + [0.0] * (nsl - len(spot_ranges))
    u, v = centres(W, H)
    d = bilinear(depth, u, v)
    inv_proj, inv_view = mat(g.camera_inverse_projection_matrix), mat(g.camera_inverse_view_matrix)
    clip = np.stack([u * 2 - 1, v * 2 - 1, d, np.ones_like(d)], -1)
    vs = apply(inv_proj, clip)
    vs = vs / vs[..., 3:4]
    world = apply(inv_view, vs)[..., :3]
    sun_pv = mat(g.sun_info.projection_matrix) @ mat(g.sun_info.view_matrix)
    sp = apply(sun_pv, np.concatenate([world, np.ones_like(d)[..., None]], -1))
    pc = sp[..., :3] / sp[..., 3:4]
    sd = bilinear(shadow, pc[..., 0] * 0.5 + 0.5, pc[..., 1] * 0.5 + 0.5)
    with np.errstate(over="ignore"):
        sun_shadow = np.clip(np.power(np.exp(g.sun_info.exponential_factor * (pc[..., 2] - sd)),
                                      g.sun_info.darkening_factor), 0.0, 1.0)
    em = bilinear(emissive, u, v)[..., :3] * g.emissive_bloom_strength
    al = bilinear(albedo, u, v)[..., :3].astype(dt)
    nn = bilinear(normal, u, v)[..., :3].astype(dt)
    occ = np.power(bilinear(npo.unorm8(ssao), u, v), g.ambient_occlussion_strength)
    sun_dir = npo.vec(g.sun_info.direction)
    direct = ((np.maximum(0.0, nn.astype(np.float64) @ -sun_dir) * sun_shadow)[..., None] * np.ones(3)).astype(dt)
    world = world.astype(dt)
    view_dir = normalize(_vec(g.camera_position, dt) - world)
    sky = d == 1.0
    ph, pw = -(-H // PATCH_H), -(-W // PATCH_W)
    reach = np.zeros((ph, pw, npl + nsl), bool)
    lit = np.zeros((ph, pw), bool)

    def patches(mask):      # any() over each 16 x 8 patch
        m = np.zeros((ph * PATCH_H, pw * PATCH_W), bool)
        m[:H, :W] = mask
        return m.reshape(ph, PATCH_H, pw, PATCH_W).any(axis=(1, 3))

    lit[:] = patches(~sky)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(npl):                       # calculate_point_light, :124-139
            L = g.point_lights[i]
            lp = _vec(L.position, dt)
            ld = normalize(lp - world)
            dist = np.linalg.norm(lp - world, axis=-1)
            att = dt(1.0) / (dist * dist)
            hw = normalize(ld + view_dir)
            diffuse = np.maximum(np.sum(nn * ld, -1), dt(0.0))
            nh = np.arccos(np.clip(np.sum(hw * nn, -1), dt(-1.0), dt(1.0)))
            term = (diffuse + np.exp(-(nh * nh))) * att * dt(L.intensity)
            if pr[i] == 0.0:                       # unlimited: np_oracle's expression, f = 1
                direct += al * _vec(L.color, dt) * term[..., None]
                reach[..., i] = lit
                continue
            w = window(np.sum((lp - world) * (lp - world), -1), pr[i], dt)
            add = direct + al * _vec(L.color, dt) * (term * w)[..., None]
            direct = np.where((w > 0)[..., None], add, direct)
            reach[..., i] = patches((w > 0) & ~sky)
        for i in range(nsl):                       # calculate_spot_light, :141-160
            L = g.spot_lights[i]
            lp = _vec(L.position, dt)
            ld = normalize(lp - world)
            sdir = _vec(L.direction, dt)
            theta = ld @ (-sdir / np.linalg.norm(sdir))
            f = np.clip((theta - dt(L.outer_cut_off)) / (dt(L.cut_off) - dt(L.outer_cut_off)), dt(0.0), dt(1.0))
            dist = np.linalg.norm(lp - world, axis=-1)
            att = dt(1.0) / (dist * dist)
            hw = normalize(ld + view_dir)
            diffuse = np.maximum(np.sum(nn * ld, -1), dt(0.0))
            nh = np.arccos(np.clip(np.sum(hw * nn, -1), dt(-1.0), dt(1.0)))
            if sr[i] != 0.0:
                f = window(np.sum((lp - world) * (lp - world), -1), sr[i], dt) * f
            add = direct + al * _vec(L.color, dt) * ((diffuse + np.exp(-(nh * nh))) * att * dt(L.intensity) * f)[..., None]
            direct = np.where((f > 0)[..., None], add, direct)
            reach[..., npl + i] = patches((f > 0) & ~sky)
    color = (direct + npo.vec(g.ambient)) * al * occ[..., None] + em
    color[sky] = bilinear(npo.unorm8(clouds), u, v)[..., :3][sky]
    if linear:
        return color, reach, lit
    out = np.concatenate([color, np.ones_like(d)[..., None]], -1)
    return out.astype(np.float16), reach, lit
