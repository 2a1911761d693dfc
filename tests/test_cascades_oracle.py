"""tests/cascades_oracle.py against np_oracle.composition (the one-cascade identity), its selection against a direct count
of compares, and the scene of the GPU test (sun_cascades_scene.py) against degeneracy. No GPU."""
import numpy as np
import pytest

import cascades_oracle as co
import np_oracle as npo
import sun_cascades_scene as scene


def bits(a):
    return np.asarray(a).view(np.uint16)


@pytest.mark.parametrize("lights", [False, True])
def test_one_cascade_of_the_sun_is_np_oracle(soc, lights):
    W, H = 64, 36
    g, gb, ssao, clouds = scene.frame_inputs(W, H)
    g = scene.copy_globals(g)
    if lights:
        scene.set_lights(g)
    ins = scene.host_inputs(gb, ssao, clouds, gb["shadow"])
    rec = soc.sun_cascades_from_sun(g, scene.S)
    got, k, kinds = co.composition(g, *ins, rec)
    want = npo.composition(g, *ins)
    assert np.array_equal(bits(got), bits(want))
    assert not k.any() and not (kinds == co.MIXED).any()


@pytest.mark.parametrize("count,lam", scene.RECORDS)
def test_selection_is_a_count_of_compares(soc, count, lam):
    W, H = 98, 56
    g, gb, _, _ = scene.frame_inputs(W, H)
    rec = scene.fit(g, count, lam)
    depth = gb["depth"].copy()
    depth[3, 5] = np.nan                            # a NaN depth: cascade 0
    depth[4, 5] = rec.split_depth[0]                # on a split: not above it
    depth[5, 5] = np.nextafter(np.float32(rec.split_depth[0]), np.float32(2.0))
    k = co.select(depth, rec)
    want = np.zeros((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            want[y, x] = sum(1 for i in range(count - 1) if np.float32(depth[y, x]) > np.float32(rec.split_depth[i]))
    assert np.array_equal(k, want)
    assert k[3, 5] == 0 and k[4, 5] == 0 and k[5, 5] == 1
    assert k.max() == count - 1


@pytest.mark.parametrize("count,lam", scene.RECORDS)
@pytest.mark.parametrize("W,H", scene.EXTENTS)
def test_scene_is_not_degenerate(soc, W, H, count, lam):
    g, gb, _, _ = scene.frame_inputs(W, H)
    rec = scene.fit(g, count, lam)
    k = co.select(gb["depth"], rec)
    kinds = co.patch_kinds(k, gb["depth"] != 1.0)
    shares, pure, mixed = scene.assert_scene(k, kinds, gb["depth"], count)
    print(f"{W}x{H} count={count}: shares {np.round(shares, 3)}, pure {pure}, mixed {mixed}")


def test_slabs_are_sampled_in_isolation(soc):
    """A slab's edge rows set to 0: only the pixels that select that slab may change."""
    W, H = 64, 36
    g, gb, ssao, clouds = scene.frame_inputs(W, H)
    rec = scene.fit(g, 3, 0.7)
    atlas = scene.atlas(g, rec)
    ref, k, _ = co.composition(g, *scene.host_inputs(gb, ssao, clouds, atlas), rec)
    spoiled = atlas.copy()
    spoiled[scene.S] = spoiled[2 * scene.S - 1] = 0.0
    got, _, _ = co.composition(g, *scene.host_inputs(gb, ssao, clouds, spoiled), rec)
    assert np.array_equal(bits(got[k != 1]), bits(ref[k != 1]))
