"""The motion oracle (tests/motion_oracle.py) judged before it judges the GPU (CPU only): with previous == current it
is the C oracle's velocity bit for bit; with a moved entity it agrees with an independent float64 computation within
the project's G-buffer bound; and it changes the velocity of the moved entity's draws only."""
import numpy as np
import pytest

import draws_oracle as D
import motion_oracle as MO
from helpers import f16_close

SIZES = ((97, 55), (160, 90))


@pytest.mark.parametrize("W,H", SIZES)
def test_previous_equal_to_current_is_the_c_oracle_bit_for_bit(soc, oracle, W, H):
    """Anchors the restatement: both the static frame the draw tests use and the moving case's frame (camera moved,
    entity 1 at phase 0.35), with None and with an equal copy as the previous array."""
    for ref in (D.reference(oracle, W, H), D.reference(oracle, W, H, frame=1, phase=MO.PHASE_CURRENT)):
        want = ref["gbuffer"]["velocity"].view(np.uint16)
        assert (want[..., :2] != 0).mean() > 0.2                                    # a velocity to compare
        copy = tuple(np.array(a, copy=True) for a in ref["scene"]["transforms"])
        for prev in (None, copy):
            got = MO.velocity(ref["g"], ref["scene"], ref["visibility"], prev)
            assert np.array_equal(got.view(np.uint16), want), (W, H, (got.view(np.uint16) != want).mean())


def _mat(m):
    return np.array(list(np.asarray(m).reshape(16)), np.float64).reshape(4, 4).T     # column-major -> math


def float64_velocity(c):
    """Independent of the oracle's chain: float64, and the OBJECT point of the pixel is formed first (perspective-correct
    barycentrics of the pixel centre) and then projected twice, with prev_vp . M_prev and with vp . M_cur.
    Returns (ys, xs, velocity (n, 2), current w, previous w)."""
    g, sc = c["g"], c["scene"]
    H, W = c["visibility"].shape
    ys, xs, d, idx = MO.pixel_triangles(sc, c["visibility"])
    xf = np.array([dr.transform for dr in sc["draws"]], np.int64)[d]
    vp, pvp = _mat(g.camera_projection_view_matrix), _mat(g.camera_previous_projection_view_matrix)
    cur = np.stack([vp @ _mat(m) for m in sc["transforms"][0]])[xf]                   # (n, 4, 4)
    prv = np.stack([pvp @ _mat(m) for m in c["previous"][0]])[xf]
    P = np.concatenate([sc["positions"][idx].astype(np.float64), np.ones(idx.shape + (1,))], -1)   # (n, 3, 4)
    clip = np.einsum("nij,nkj->nki", cur, P)                                          # (n, 3 vertices, 4)
    # 2DH: the pixel centre's barycentrics over (X, Y, w) are the perspective-correct ones
    V = np.stack([(clip[..., 0] * 0.5 + clip[..., 3] * 0.5) * W, (clip[..., 1] * 0.5 + clip[..., 3] * 0.5) * H,
                  clip[..., 3]], -1)                                                  # (n, 3, 3)
    px = np.stack([xs + 0.5, ys + 0.5, np.ones(len(xs))], -1)
    b = np.linalg.solve(np.swapaxes(V, 1, 2), px[..., None])[..., 0]                   # sum_k b_k V_k = s (x, y, 1)
    b = b / b.sum(1, keepdims=True)
    obj = np.einsum("nk,nkj->nj", b, P)
    pc, pp = np.einsum("nij,nj->ni", cur, obj), np.einsum("nij,nj->ni", prv, obj)
    vel = (pc[:, :2] / pc[:, 3:] * 0.5 + 0.5) - (pp[:, :2] / pp[:, 3:] * 0.5 + 0.5)
    return ys, xs, vel, pc[:, 3], pp[:, 3]


@pytest.mark.parametrize("W,H", SIZES)
def test_moving_case_against_float64(soc, oracle, W, H):
    """Frame 1's globals, current = entities_for(0.35), previous = entities_for(0.0). The oracle's RGBA16F velocity is
    within helpers.f16_close (the G-buffer bound) of the float64 value on at least 0.9999 of the values. Pixels whose
    interpolated current or previous w lies below the near distance are excluded (a triangle through the near plane
    divides by a w near zero, where float32 and float64 legitimately part); they are at most 1 % of the covered ones."""
    c = MO.case(oracle, W, H)
    ys, xs, vel, w_cur, w_prev = float64_velocity(c)
    near = float(c["g"].camera_near_clip)
    assert near > 0
    keep = (w_cur >= near) & (w_prev >= near)
    excluded = 1.0 - keep.mean()
    got = c["velocity"][ys, xs, :2][keep]
    ok = f16_close(got, vel[keep].astype(np.float16))
    print(f"{W}x{H}: {len(ys)} covered pixels, excluded {excluded:.5f}, within tolerance on {ok.mean():.6f}")
    assert excluded <= 0.01, excluded
    assert ok.mean() >= 0.9999, ok.mean()
    # .zw and the empty pixels carry the clear values
    assert (c["velocity"][..., 2] == 0).all() and (c["velocity"][..., 3] == 1).all()
    assert (c["velocity"][c["draw"] < 0][:, :2] == 0).all()


@pytest.mark.parametrize("W,H", SIZES)
def test_only_the_moved_entity_changes(soc, oracle, W, H):
    c = MO.case(oracle, W, H)
    moving = np.isin(c["draw"], MO.moving_draws(c["scene"]))
    others = (c["draw"] >= 0) & ~moving
    assert moving.sum() >= 50 and others.sum() >= 50
    a, b = c["velocity"].view(np.uint16), c["reference_velocity"].view(np.uint16)
    differs = (a != b).any(-1)
    assert differs[moving].mean() > 0.5, differs[moving].mean()
    assert not differs[others].any() and not differs[c["draw"] < 0].any()
