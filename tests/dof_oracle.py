"""dof_oracle — numpy restatement of the reference's depth-of-field task chain (TEST INFRASTRUCTURE).

Written from src/graphics/tasks/depth_of_field.inl (BlitImageToImage :16-48, MipMapping :55-88, the DepthOfField fragment
shader :176-199) and renderer.cpp:346, 463-488 (the RGBA16F image with floor(log2(max(W, H))) + 1 levels; the sampler:
trilinear, REPEAT, anisotropy 16, max_lod = L) under the project's sampling contract: 8-bit sub-texel
weights, lerp(a, b, w) = a (1 - w) + b w, bilinear = lerp(lerp(t00, t01, wx), lerp(t10, t11, wx), wy).

Every operation is an explicit elementwise numpy operation in the dtype `T`, so with T = float32 each rounds once to
fp32 in the order written here; that order is the contract csrc/dof.hip follows. T = float64 runs the same formulas in
double (np.log2 for the deterministic log2): the difference is the pass's sensitivity to rounding.

The chain:  level 0 = the colour's texels; level k = LINEAR blit of level k - 1 (clamp to edge; destination texel x
            samples ((2x + 1) n_src) / (2 n_dst) - 0.5), rounded to float16 nearest-even.
The pass:   u = (x + 0.5) / W, v = (y + 0.5) / H, d = depth[y, x]; not (d < 1): the level-0 texel, all four halves.
            od  = (-far near) / (d (far - near) - far)
            coc = |(A (F (od - P))) / (od (P - F))|, max_coc = |(A (F (far - P))) / (od (P - F))|, c = coc / max_coc
            rho = sqrt((c W)^2 + (c H)^2); lq = clamp(floor(clamp(log2 rho, -64, 64) 256 + 0.5), 0, (L - 1) 256), 0 when
            not (0 < rho <= 3.4e38); l0 = lq >> 8, l1 = min(l0 + 1, L - 1), f = (lq & 255) / 256
            taps (u + 1/W, v), (u - 1/W, v), (u, v + 1/H), (u, v - 1/H): REPEAT bilinear of level l0, blended with
            level l1 as lerp(s0, s1, f) when lq & 255 != 0
            rgb = ((t0 0.25 + t1 0.25) + t2 0.25) + t3 0.25, a = 1, rounded to float16 nearest-even.
"""
from __future__ import annotations

import numpy as np


def level_count(W, H):
    return int(max(W, H)).bit_length()        # floor(log2(max(W, H))) + 1


def level_shapes(W, H):
    """[(h, w)] of every level: max(1, n // 2) per step."""
    out = [(H, W)]
    while out[-1] != (1, 1):
        h, w = out[-1]
        out.append((max(1, h // 2), max(1, w // 2)))
    assert len(out) == level_count(W, H)
    return out


def _lerp(a, b, w, T):
    return a * (T(1.0) - w) + b * w


def _bilerp(img, x0, x1, wx, y0, y1, wy, T):
    """img (h, w, C) in T; the index / weight arrays broadcast against each other; returns (..., C)."""
    wx, wy = wx[..., None], wy[..., None]
    return _lerp(_lerp(img[y0, x0], img[y0, x1], wx, T), _lerp(img[y1, x0], img[y1, x1], wx, T), wy, T)


# ---------------------------------------------------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------------------------------------------------
def _blit_axis(n_dst, n_src, T):
    """texture.hip's blit_axis for every destination texel: taps i0, i1 and the weight of i1 (a multiple of 1/256)."""
    x = np.arange(n_dst)
    t = ((2 * x + 1).astype(T) * T(n_src)) / T(2 * n_dst) - T(0.5)
    fx = np.floor(t * T(256.0) + T(0.5)).astype(np.int64)
    i = fx >> 8
    w = (fx & 255).astype(T) * T(1.0 / 256.0)
    lo, hi = i < 0, i >= n_src - 1
    i = np.where(lo, 0, np.where(hi, n_src - 2, i))
    w = np.where(lo, T(0.0), np.where(hi, T(1.0), w))
    if n_src == 1:
        i, w = np.zeros_like(i), np.zeros_like(w)
    return i, np.minimum(i + 1, n_src - 1), w


def blit(src, dtype=np.float32):
    """One MipMapping task: the float16 (h, w, 4) level below `src`."""
    T = dtype
    sh, sw = src.shape[:2]
    dh, dw = max(1, sh // 2), max(1, sw // 2)
    x0, x1, wx = _blit_axis(dw, sw, T)
    y0, y1, wy = _blit_axis(dh, sh, T)
    with np.errstate(all="ignore"):
        out = _bilerp(src.astype(T), x0[None, :], x1[None, :], wx[None, :], y0[:, None], y1[:, None], wy[:, None], T)
        return out.astype(np.float16)


def chain(color, dtype=np.float32):
    """BlitImageToImage + every MipMapping task: the list of float16 levels of an (H, W, 4) float16 colour image."""
    levels = [np.array(color, np.float16)]
    while levels[-1].shape[:2] != (1, 1):
        levels.append(blit(levels[-1], dtype))
    return levels


# ---------------------------------------------------------------------------------------------------------------------
# the pass
# ---------------------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """fmaf on float32 values: the product is exact in float64; the sum's double rounding is far below the oracle's use
    of the result (an lq step is 1/256 of a level)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def det_log2(x):
    """luminance.hpp's det_log2 (soc_oracle_log2's operation sequence) for positive finite float32 x."""
    f32 = np.float32
    x = np.asarray(x, f32)
    u = x.view(np.uint32).astype(np.int64)
    sub = u < 0x00800000
    xs = np.where(sub, x * f32(8388608.0), x).astype(f32)
    u = xs.view(np.uint32).astype(np.int64)
    e = np.where(sub, -23, 0) + (u >> 23) - 127
    m = ((u & 0x007FFFFF) | 0x3F800000).astype(np.uint32).view(f32)
    big = m > f32(1.41421356)
    m = np.where(big, m * f32(0.5), m).astype(f32)
    e = e + big
    f = m - f32(1.0)
    s = f / (f32(2.0) + f)
    s2 = s * s
    p = _fma32(s2, f32(1.0) / f32(11.0), f32(1.0) / f32(9.0))
    p = _fma32(s2, p, f32(1.0) / f32(7.0))
    p = _fma32(s2, p, f32(1.0) / f32(5.0))
    p = _fma32(s2, p, f32(1.0) / f32(3.0))
    p = _fma32(s2, p, f32(1.0))
    ln = (f32(2.0) * s) * p
    return _fma32(ln, f32(1.44269504088896341), e.astype(f32))


def _axis_repeat(u, n, T):
    """axis_repeat_any: REPEAT taps i0, i1 (wrapping around) and the weight of i1."""
    t = u * T(n)
    t = t - T(0.5)
    t = np.fmin(np.fmax(t, T(-4194304.0)), T(4194304.0))
    fx = np.floor(t * T(256.0) + T(0.5)).astype(np.int64)
    r = (fx >> 8) % n
    return r, (r + 1) % n, (fx & 255).astype(T) * T(1.0 / 256.0)


def _tap(level, u, v, T):
    """rgb of one bilinear REPEAT tap of a float16 level at the coordinate arrays (u, v)."""
    h, w = level.shape[:2]
    x0, x1, wx = _axis_repeat(u, w, T)
    y0, y1, wy = _axis_repeat(v, h, T)
    return _bilerp(level[..., :3].astype(T), x0, x1, wx, y0, y1, wy, T)


def lod_q(g, depth, W, H, dtype=np.float32):
    """lq (int64, in 1/256 levels) of the pixels with the given depths (all < 1) of a W x H frame."""
    T = dtype
    L = level_count(W, H)
    near, far = T(np.float32(g.camera_near_clip)), T(np.float32(g.camera_far_clip))
    A, F, P = T(np.float32(g.aperture)), T(np.float32(g.focal_length)), T(np.float32(g.plane_in_focus))
    d = depth.astype(T)
    with np.errstate(all="ignore"):
        od = (-far * near) / (d * (far - near) - far)
        den = od * (P - F)
        coc = np.abs((A * (F * (od - P))) / den)
        max_coc = np.abs((A * (F * (far - P))) / den)
        c = coc / max_coc
        ax, ay = c * T(W), c * T(H)
        rho = np.sqrt(ax * ax + ay * ay)
        ok = (rho > 0) & (rho <= T(np.float32(3.4e38)))
        safe = np.where(ok, rho, T(1.0))
        lam = det_log2(safe) if T is np.float32 else np.log2(safe)
        lam = np.fmin(np.fmax(lam, T(-64.0)), T(64.0))
        lq = np.clip(np.floor(lam * T(256.0) + T(0.5)).astype(np.int64), 0, (L - 1) * 256)
    return np.where(ok, lq, 0)


def depth_of_field(g, depth, levels, dtype=np.float32, lq_offset=0):
    """DepthOfFieldTask on host arrays: depth (H, W) float32, levels = chain(color). Returns (rgba float16 (H, W, 4), lq
    int32 (H, W), -1 on the copied pixels). lq_offset (-1, 0 or +1) moves every geometry pixel's lq by that many 1/256
    steps (clamped to the chain): the neighbouring answers a last-place difference in the lod can give."""
    T = dtype
    H, W = depth.shape
    L = len(levels)
    assert levels[0].shape[:2] == (H, W) and L == level_count(W, H)
    out = np.array(levels[0], np.float16)                   # :196-198, the copied pixels
    lq_img = np.full((H, W), -1, np.int32)
    with np.errstate(invalid="ignore"):
        ys, xs = np.nonzero(depth < np.float32(1.0))
    if ys.size == 0:
        return out, lq_img
    lq = np.clip(lod_q(g, depth[ys, xs], W, H, T) + int(lq_offset), 0, (L - 1) * 256)
    lq_img[ys, xs] = lq
    l0 = lq >> 8
    l1 = np.minimum(l0 + 1, L - 1)
    frac = lq & 255
    f = frac.astype(T) * T(1.0 / 256.0)
    u = (xs.astype(T) + T(0.5)) / T(W)
    v = (ys.astype(T) + T(0.5)) / T(H)
    ox, oy = T(1.0) / T(W), T(1.0) / T(H)
    taps = [(u + ox, v), (u - ox, v), (u, v + oy), (u, v - oy)]
    q = T(0.25)
    rgb = np.zeros((ys.size, 3), T)
    with np.errstate(all="ignore"):
        for k in range(L):
            m = l0 == k
            if m.any():
                t = [_tap(levels[k], tu[m], tv[m], T) for tu, tv in taps]
                b = m & (frac != 0)
                if b.any():
                    sub = b[m]                               # within the level's pixels: those that blend
                    kb = int(l1[b][0])                       # l1 is a function of l0
                    for i, (tu, tv) in enumerate(taps):
                        t[i][sub] = _lerp(t[i][sub], _tap(levels[kb], tu[b], tv[b], T), f[b][:, None], T)
                rgb[m] = ((t[0] * q + t[1] * q) + t[2] * q) + t[3] * q
        out[ys, xs, :3] = rgb.astype(np.float16)
    out[ys, xs, 3] = np.float16(1.0)
    return out, lq_img
