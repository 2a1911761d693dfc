"""The ScreenSpaceReflection oracle (tests/ssr_oracle.py) on scenes whose result can be worked out by hand, and the
rounding sensitivity of the pass on the inputs of the GPU parity test (CPU only).

The hand-checkable scenes are planes seen by a perspective camera at the view-space origin (identity view matrix). The
depth of a plane is affine in screen space, so the bilinear depth tap is exact on it and the march can be predicted
without the depth image: the probe at view position p sees, along its own screen ray, the nearest plane at t p
(t > 0), so delta = |p.z| - t |p.z|. `_march` does that in scalar float64, independently of the oracle's code."""
import numpy as np
import pytest

import helpers
import ssr_inputs
import ssr_oracle

W, H = 64, 48
WALL_RGB, FLOOR_RGB = (0.25, 0.5, 0.75), (0.875, 0.125, 0.0625)     # exact in RGBA16F


def _mat(field):
    return np.array(list(field), np.float64).reshape(4, 4).T          # M[row, col]


def _nearest(planes, d):
    """Smallest t > 0 with t d on one of the planes (axis, coordinate); (inf, None) when the ray meets none."""
    best, which = np.inf, None
    for k, (axis, c) in enumerate(planes):
        if d[axis] != 0.0 and c / d[axis] > 0.0 and c / d[axis] < best:
            best, which = c / d[axis], k
    return best, which


def _scene(soc, planes, far=1000.0):
    """Globals with an identity view matrix and the G-buffer of `planes` [(axis, coordinate, normal, rgb)]: pixels
    whose ray meets no plane are sky (depth 1, normal and albedo 0)."""
    g = helpers.globals_for(W, H)
    g.camera_view_matrix[:] = [float(v) for v in np.eye(4).reshape(16)]
    P, IP = _mat(g.camera_projection_matrix), _mat(g.camera_inverse_projection_matrix)
    depth = np.ones((H, W), np.float32)
    normal = np.zeros((H, W, 4), np.float16)
    albedo = np.zeros((H, W, 4), np.float16)
    rays = np.zeros((H, W, 3))
    for y in range(H):
        for x in range(W):
            p = IP @ np.array([(x + 0.5) / W * 2 - 1, (y + 0.5) / H * 2 - 1, 0.5, 1.0])
            d = p[:3] / p[3]                                          # a point of the pixel's ray from the eye
            rays[y, x] = d
            t, k = _nearest([(a, c) for a, c, _, _ in planes], d)
            if k is None:
                continue
            c = P @ np.append(t * d, 1.0)
            depth[y, x] = c[2] / c[3]
            normal[y, x, :3] = planes[k][2]
            albedo[y, x, :3] = planes[k][3]
            albedo[y, x, 3] = 1.0
    mr = np.zeros((H, W, 4), np.float16)
    mr[..., 0], mr[..., 1] = 0.5, 0.8
    return g, depth, normal, albedo, mr, rays


def _march(planes, pos, n, far=1000.0):
    """The shader's march (screen_space_reflection.inl:119-162) in scalar float64 against the analytic planes. Returns
    (steps, index of the plane hit or None, smallest distance of any |delta| from a branch threshold, largest mp.z)."""
    geo = [(a, c) for a, c, _, _ in planes]

    def delta_at(mp):
        if mp[2] >= 0.0:                   # behind the eye: only used with a screen-filling plane of constant depth
            return abs(mp[2]) - abs(geo[0][1]), 0
        t, k = _nearest(geo, mp)
        return (abs(mp[2]) - t * abs(mp[2]), k) if k is not None else (abs(mp[2]) - far, None)

    n = np.asarray(n, np.float64)
    r = pos - 2.0 * np.dot(n, pos) * n
    r /= np.linalg.norm(r)
    step = 0.5 * r
    mp = pos + step
    margin, zmax, i = np.inf, mp[2], 0
    delta = 0.0
    while i < 50:
        delta, k = delta_at(mp)
        margin = min(margin, abs(abs(delta) - 0.05), abs(delta))
        zmax = max(zmax, mp[2])
        if abs(delta) < 0.05:
            return i, k, margin, zmax
        if delta > 0:
            break
        mp = mp + step
        step = step * 1.05
        i += 1
    while i < 50:
        step = step * 0.5
        mp = mp - step * np.sign(delta)
        delta, k = delta_at(mp)
        margin = min(margin, abs(abs(delta) - 0.05), abs(delta))
        if abs(delta) < 0.05:
            return i, k, margin, zmax
        i += 1
    return 50, None, margin, zmax


FLOOR = (1, -1.5, (0.0, 1.0, 0.0), FLOOR_RGB)       # y = -1.5, facing up
WALL = (2, -8.0, (0.0, 0.0, 1.0), WALL_RGB)         # z = -8, facing the camera


def _floor_pixel(depth, normal, rays, column, view_z):
    """The floor pixel of `column` whose view-space z is nearest to view_z."""
    ys = [y for y in range(H) if normal[y, column, 1] == 1.0]
    assert ys
    z = {y: rays[y, column, 2] * (FLOOR[1] / rays[y, column, 1]) for y in ys}
    return min(ys, key=lambda y: abs(z[y] - view_z))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_mirror_floor_reflects_the_wall(soc, dtype):
    """A floor pixel 3 units ahead reflects the wall 5 units further on: the first loop overshoots the wall after about
    eight growing steps (0.5 x 1.05^k sums to 5 at k = 8), the binary search converges onto it, and the colour is the
    wall's albedo. The step count is the analytic march's."""
    planes = [FLOOR, WALL]
    g, depth, normal, albedo, mr, rays = _scene(soc, planes)
    x = W // 2 + 3
    y = _floor_pixel(depth, normal, rays, x, -3.0)
    pos = rays[y, x] * (FLOOR[1] / rays[y, x, 1])
    want, plane, margin, _ = _march(planes, pos, FLOOR[2])
    assert plane == 1 and 5 <= want <= 20, (want, plane)
    assert margin > 1e-3, margin             # no branch of this pixel's march is near a threshold
    rgba, steps = ssr_oracle.screen_space_reflection(g, depth, normal, albedo, mr, dtype)
    assert steps[y, x] == want
    assert rgba[y, x].tolist() == [*WALL_RGB, 1.0]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_non_metal_pixel_copies_its_albedo(soc, dtype):
    g, depth, normal, albedo, mr, rays = _scene(soc, [FLOOR, WALL])
    x, y = 11, _floor_pixel(depth, normal, rays, 11, -3.0)
    mr[y, x, 1] = 0.0078                      # below the shader's 0.01
    mr[y, x + 1, 1] = 0.0101                  # above it: marches
    albedo[y, x] = [0.3, 0.6, 0.9, 0.5]
    rgba, steps = ssr_oracle.screen_space_reflection(g, depth, normal, albedo, mr, dtype)
    assert steps[y, x] == ssr_oracle.STEPS_COPY == 255
    assert rgba[y, x].tolist() == [*albedo[y, x, :3].tolist(), 1.0]
    assert steps[y, x + 1] != 255
    assert (steps != 255).sum() == W * H - 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ray_into_the_sky_misses(soc, dtype):
    """A floor with nothing behind it: a steep ray near the screen's edge rises into the sky (depth 1: far away, delta
    stays negative for all 50 iterations). Sky pixels (zero normal: a NaN reflection) can only miss. Alpha is 1 on every
    pixel, and a miss is (0, 0, 0, 1): the shader's albedo fallback never fires."""
    planes = [FLOOR]
    g, depth, normal, albedo, mr, rays = _scene(soc, planes)
    x = W // 2
    y = _floor_pixel(depth, normal, rays, x, -1.6)
    pos = rays[y, x] * (FLOOR[1] / rays[y, x, 1])
    want, plane, margin, _ = _march(planes, pos, FLOOR[2])
    assert want == 50 and plane is None and margin > 1e-3
    rgba, steps = ssr_oracle.screen_space_reflection(g, depth, normal, albedo, mr, dtype)
    assert steps[y, x] == ssr_oracle.STEPS_MISS == 50
    assert rgba[y, x].tolist() == [0.0, 0.0, 0.0, 1.0]
    sky = depth == 1.0
    assert sky.any() and (steps[sky] == 50).all()
    assert (rgba[sky] == np.array([0, 0, 0, 1], np.float16)).all()
    assert (rgba[..., 3] == 1.0).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ray_behind_the_eye_misses(soc, dtype):
    """A screen-filling wall 60 units away throws every ray back past the camera: the march's 104 units of reach take it
    behind the eye (view z > 0, clip w < 0, screen positions far outside the image, clamped to its edge), where
    |z| stays below the wall's 60: delta is negative throughout and every pixel is a miss."""
    far_wall = (2, -60.0, (0.0, 0.0, 1.0), WALL_RGB)
    g, depth, normal, albedo, mr, rays = _scene(soc, [far_wall])
    x, y = W // 2 - 5, H // 2 + 4
    pos = rays[y, x] * (far_wall[1] / rays[y, x, 2])
    want, _, margin, zmax = _march([far_wall], pos, far_wall[2])
    assert want == 50 and zmax > 10.0 and margin > 0.4
    rgba, steps = ssr_oracle.screen_space_reflection(g, depth, normal, albedo, mr, dtype)
    assert (steps == 50).all()
    assert (rgba == np.array([0, 0, 0, 1], np.float16)).all()


# Float64 against float32 on the inputs of the GPU parity test: the share of pixels where a different rounding alone
# changes the result (a branch of the 50 dependent iterations flips). It justifies that test's 0.5 % cap.
SENSITIVITY_CAP = 0.0025


@pytest.mark.parametrize("name", list(ssr_inputs.INPUTS))
def test_rounding_sensitivity(name):
    ref_rgba, ref_steps = ssr_inputs.reference(name)
    rgba, steps = ssr_inputs.run_oracle(name, np.float64)
    bad = ssr_inputs.disagreeing(rgba, steps, ref_rgba, ref_steps)
    marching = ref_steps != 255
    print(f"ssr sensitivity {name}: {int(bad.sum())} of {bad.size} px differ ({bad.mean():.4%}); "
          f"copies {(~marching).mean():.1%}, misses {(ref_steps == 50).mean():.1%}, hits {(ref_steps < 50).mean():.1%}")
    assert (rgba[..., 3] == 1.0).all() and (ref_rgba[..., 3] == 1.0).all()
    assert ((steps == 255) == (ref_steps == 255)).all()
    assert bad.mean() <= SENSITIVITY_CAP, (name, int(bad.sum()), bad.size)
