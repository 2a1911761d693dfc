"""ssr_oracle — numpy restatement of the reference's ScreenSpaceReflection fragment shader (TEST INFRASTRUCTURE).

Written from the GLSL (src/graphics/tasks/screen_space_reflection.inl:88-183, cited per function) under the project's
sampling contract: `linear_sampler` taps are clamp-to-edge with 8-bit sub-texel weights, a NaN coordinate
selects texel 0, and a tap at a pixel centre of an image of the target's extent is that texel.

Every operation is an explicit elementwise numpy operation in the dtype `T` (no `@`, einsum or dot: BLAS may reorder or
fuse), so with T = float32 each one rounds once to fp32, in the order written here. That order is the contract the HIP
kernel (csrc/ssr.hip) follows; float32 is the yardstick. T = float64 runs the same formulas (the same fp32 constants,
widened) in double: the difference between the two runs is the pass's sensitivity to rounding.

Operation order (column-major m[col * 4 + row], sums left to right):
  M * (x, y, z, 1) row r  = ((m[r] x + m[4 + r] y) + m[8 + r] z) + m[12 + r]
  mat3(M) * v      row r  = (m[r] x + m[4 + r] y) + m[8 + r] z
  dot(a, b)               = (a.x b.x + a.y b.y) + a.z b.z
  normalize(v)            = v / sqrt(dot(v, v)), one division per component
  reflect(I, N)           = I - (2 dot(N, I)) N
  view z of (uv, d)       = row 2 / row 3 of IP * (uv 2 - 1, d, 1)
  screen of p             = (row 0 / row 3) 0.5 + 0.5, (row 1 / row 3) 0.5 + 0.5 of P * (p, 1)
  bilinear tap            = lerp(lerp(t00, t01, wx), lerp(t10, t11, wx), wy), lerp(a, b, w) = a (1 - w) + b w
"""
from __future__ import annotations

import numpy as np

ITERATIONS = 50          # iterationCount, :98
STEPS_MISS = 50          # `steps` of a ray that found nothing
STEPS_COPY = 255         # `steps` of a pixel the shader copies (metallic < 0.01, :171-174)
RAY_STEP = np.float32(0.5)         # rayStep, :97
DISTANCE_BIAS = np.float32(0.05)   # distanceBias, :99
STEP_GROWTH = np.float32(1.05)     # :144
METALLIC_MIN = np.float32(0.01)    # :171


def metallic_roughness_pattern(H, W, seed=7):
    """The test inputs' metallic-roughness image (RGBA16F; .x roughness, .y metallic as the shader reads them, :169-171):
    roughness uniform random, metallic 0.8 except 0 on every fourth 8x8 block of a diagonal checker, so a quarter of the
    pixels are copies and copies and marching pixels share waves."""
    rng = np.random.default_rng(seed)
    mr = np.zeros((H, W, 4), np.float32)
    mr[..., 0] = rng.uniform(0.0, 1.0, (H, W))
    by, bx = np.mgrid[0:H, 0:W] // 8
    mr[..., 1] = np.where((bx + by) % 4 == 0, 0.0, 0.8)
    return mr.astype(np.float16)


def _axis(u, n, T):
    """axis_clamp of the sampling contract: left tap, right tap and the right tap's weight (a multiple of 1/256)."""
    t = u * T(n)
    t = t - T(0.5)
    t = np.fmin(np.fmax(t, T(-2.0)), T(n) + T(1.0))      # NaN -> -2 -> texel 0
    fx = np.floor(t * T(256.0) + T(0.5)).astype(np.int64)
    i = fx >> 8
    w = (fx & 255).astype(T) * T(1.0 / 256.0)
    lo, hi = i < 0, i >= n - 1
    i = np.where(lo, 0, np.where(hi, n - 2, i))
    w = np.where(lo, T(0.0), np.where(hi, T(1.0), w))
    if n == 1:
        i, w = np.zeros_like(i), np.zeros_like(w)
    return i, np.minimum(i + 1, n - 1), w


def _lerp(a, b, w, T):
    return a * (T(1.0) - w) + b * w


def _sample(img, u, v, T):
    """texture(sampler2D(img, linear_sampler), (u, v)) of an (H, W[, C]) image, computed in T."""
    h, w = img.shape[:2]
    x0, x1, wx = _axis(u, w, T)
    y0, y1, wy = _axis(v, h, T)
    a = img.astype(T)
    if a.ndim == 3:
        wx, wy = wx[..., None], wy[..., None]
    return _lerp(_lerp(a[y0, x0], a[y0, x1], wx, T), _lerp(a[y1, x0], a[y1, x1], wx, T), wy, T)


def _row(m, r, x, y, z):
    return ((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r]


def _row3(m, r, x, y, z):
    return (m[r] * x + m[4 + r] * y) + m[8 + r] * z


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _normalize(v):
    length = np.sqrt(_dot(v, v))
    return [v[0] / length, v[1] / length, v[2] / length]


def _sign(x, T):
    """(x > 0) - (x < 0): NaN gives 0."""
    return (x > 0).astype(T) - (x < 0).astype(T)


def screen_space_reflection(g, depth, normal, albedo, metallic_roughness, dtype=np.float32):
    """The pass on host arrays: depth (H, W) float32, the others (H, W, 4) float16. Returns (rgba, steps): the RGBA16F
    target as float16 (H, W, 4) and the uint8 step image (0..49 the iteration of the hit, 50 a miss, 255 a copy)."""
    T = dtype
    H, W = depth.shape
    P = np.array(list(g.camera_projection_matrix), np.float32).astype(T)
    IP = np.array(list(g.camera_inverse_projection_matrix), np.float32).astype(T)
    V = np.array(list(g.camera_view_matrix), np.float32).astype(T)
    bias, half, growth = T(DISTANCE_BIAS), T(RAY_STEP), T(STEP_GROWTH)

    out = np.zeros((H, W, 4), T)
    out[..., 3] = T(1.0)                                   # :172, :179 (the :180 fallback never fires: alpha is 1)
    steps = np.full((H, W), STEPS_MISS, np.uint8)

    # :169-174 copy path (pixel-centre taps of same-size images are texel loads)
    copy = metallic_roughness[..., 1].astype(np.float32) < METALLIC_MIN
    out[copy, :3] = albedo[copy, :3].astype(T)
    steps[copy] = STEPS_COPY

    ys, xs = np.nonzero(~copy)
    if ys.size == 0:
        return out.astype(np.float16), steps
    with np.errstate(all="ignore"):
        u = (xs.astype(T) + T(0.5)) / T(W)
        v = (ys.astype(T) + T(0.5)) / T(H)
        d = depth[ys, xs].astype(T)
        # get_view_position_from_depth, :88-95
        cx, cy = u * T(2.0) - T(1.0), v * T(2.0) - T(1.0)
        pw = _row(IP, 3, cx, cy, d)
        pos = [_row(IP, 0, cx, cy, d) / pw, _row(IP, 1, cx, cy, d) / pw, _row(IP, 2, cx, cy, d) / pw]
        # :177-178
        n = normal[ys, xs].astype(T)
        nv = _normalize([_row3(V, r, n[:, 0], n[:, 1], n[:, 2]) for r in range(3)])
        k = T(2.0) * _dot(nv, pos)
        refl = _normalize([pos[c] - k * nv[c] for c in range(3)])
        # ssr(), :119-162
        step = [half * refl[c] for c in range(3)]
        mp = [pos[c] + step[c] for c in range(3)]

        def probe(mp):
            # generateProjectedPosition, :113-117
            cw = _row(P, 3, mp[0], mp[1], mp[2])
            sx = (_row(P, 0, mp[0], mp[1], mp[2]) / cw) * T(0.5) + T(0.5)
            sy = (_row(P, 1, mp[0], mp[1], mp[2]) / cw) * T(0.5) + T(0.5)
            dd = _sample(depth, sx, sy, T)
            ex, ey = sx * T(2.0) - T(1.0), sy * T(2.0) - T(1.0)
            vz = _row(IP, 2, ex, ey, dd) / _row(IP, 3, ex, ey, dd)
            return sx, sy, np.abs(mp[2]) - np.abs(vz)

        m = ys.size
        i = np.zeros(m, np.int64)
        binary = np.zeros(m, bool)       # the lane is in the second loop (:147-159)
        live = np.ones(m, bool)
        sgn = np.zeros(m, T)
        while live.any():
            # second loop's step before its probe, :149-150
            for c in range(3):
                step[c] = np.where(binary, step[c] * half, step[c])
                mp[c] = np.where(binary, mp[c] - step[c] * sgn, mp[c])
            sx, sy, delta = probe(mp)
            hit = live & (np.abs(delta) < bias)                      # :131, :156
            if hit.any():
                out[ys[hit], xs[hit], :3] = _sample(albedo[..., :3], sx[hit], sy[hit], T)
                steps[ys[hit], xs[hit]] = i[hit]
            live &= ~hit
            sgn = np.where(live, _sign(delta, T), sgn)
            brk = live & ~binary & (delta > 0)                       # :135-137: leaves the first loop, i unchanged
            adv = live & ~binary & ~brk                              # :139-144
            f = T(1.0) - half * np.maximum(sgn, T(0.0))
            for c in range(3):
                s1 = step[c] * f
                step[c] = np.where(adv, s1, step[c])
                mp[c] = np.where(adv, mp[c] + s1 * (-sgn), mp[c])
                step[c] = np.where(adv, step[c] * growth, step[c])
            i = np.where(live & ~brk, i + 1, i)
            binary |= brk
            live &= i < ITERATIONS                                   # a first loop that ran out leaves no second loop
    return out.astype(np.float16), steps
