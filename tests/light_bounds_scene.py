"""The lights of the bounded-lights tests (test_lights_oracle.py, test_gpu_light_bounds.py): six point and six spot lights
in the atrium in front of helpers.SPONZA_CAMERA with mixed ranges, chosen on the CPU oracle so that the culling has
something to do at every test extent: one light reaches no 16 x 8 patch, some reach every lit patch, and between 20 %
and 80 % of the (patch, light) pairs are empty (the GPU test asserts all three from lights_oracle's table)."""
import numpy as np

# (position, colour, intensity, range): range 0 = unlimited
POINTS = [
    ((-10.0, 2.0, 0.5), (1.0, 0.8, 0.6), 3.0, 0.0),      # unlimited: reaches every lit patch
    ((-11.5, 0.8, -1.0), (0.6, 0.9, 1.0), 2.0, 5.0),     # near the floor, left of the view
    ((-9.0, 3.5, 2.0), (1.0, 0.5, 0.4), 4.0, 5.0),
    ((-6.0, 1.5, 0.0), (0.7, 1.0, 0.7), 3.0, 6.0),
    ((-12.0, 2.2, 0.3), (1.0, 1.0, 0.9), 1.5, 40.0),     # a range beyond the scene: a window near 1 everywhere
    ((40.0, 30.0, 40.0), (1.0, 1.0, 1.0), 9.0, 5.0),     # far outside: reaches no patch
]
# (position, direction, colour, intensity, cut_off, outer_cut_off, range)
SPOTS = [
    ((-8.0, 4.0, -1.0), (0.3, -1.0, 0.1), (0.5, 0.7, 1.0), 5.0, 0.9, 0.6, 0.0),        # unlimited, cone only
    ((-10.0, 5.0, 1.0), (0.0, -1.0, 0.0), (1.0, 0.9, 0.7), 6.0, 0.97, 0.90, 6.0),
    ((-11.0, 3.0, 0.3), (1.0, -0.3, 0.0), (0.8, 0.8, 1.0), 4.0, 0.92, 0.80, 8.0),      # along the view direction
    ((-4.0, 4.5, 0.5), (-0.2, -1.0, 0.2), (1.0, 0.6, 0.6), 5.0, 0.95, 0.85, 5.0),
    ((-13.0, 2.2, 0.3), (-1.0, 0.0, 0.0), (0.6, 1.0, 0.8), 5.0, 0.9, 0.7, 0.0),         # behind the camera, pointing away
    ((-9.0, 1.0, -2.0), (0.0, 0.2, 1.0), (0.9, 0.7, 1.0), 3.0, 0.9, 0.6, 6.0),
]
POINT_RANGES = [p[3] for p in POINTS]
SPOT_RANGES = [s[6] for s in SPOTS]


def set_lights(g):
    g.point_light_count, g.spot_light_count = len(POINTS), len(SPOTS)
    for L, (pos, col, inten, _) in zip(g.point_lights, POINTS):
        L.position[:] = pos
        L.color[:] = col
        L.intensity = inten
    for L, (pos, dirn, col, inten, cut, outer, _) in zip(g.spot_lights, SPOTS):
        L.position[:] = pos
        L.direction[:] = dirn
        L.color[:] = col
        L.intensity = inten
        L.cut_off, L.outer_cut_off = cut, outer
    return g


def frame_inputs(W, H):
    """g (with the lights), the G-buffer of helpers.sponza_inputs, and seeded AO and clouds images."""
    from helpers import sponza_inputs
    g, gb = sponza_inputs(W, H, shadow_size=256)
    set_lights(g)
    rng = np.random.default_rng(W * 1000 + H)
    ssao = rng.integers(120, 256, (H // 2, W // 2), dtype=np.uint8)
    clouds = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    return g, gb, ssao, clouds
