"""Per-object motion vectors of draw scenes on the GPU (-m gpu): soc_gbuffer_resolve_draws_motion and the render graph's
GBufferGeneration with soc_renderer_set_draw_motion, against the existing resolve (bit for bit wherever the previous
model matrix equals the current one) and against the motion oracle (tests/motion_oracle.py, itself proved by
tests/test_motion_oracle.py).

Tolerances: equality is torch.equal; the moved entity's velocity is within helpers.f16_close (1e-3 + 2e-3 |ref|, the
G-buffer's RGBA16F bound) of the oracle on at least 0.9999 of the values. The shared scene's slot ranges of 255 and 257
vertices straddle workgroups and waves, so both the per-wave LDS path and the per-lane path of the vertex kernel run.
"""
import numpy as np
import pytest
import torch

import draws_oracle as D
import motion_oracle as MO
from helpers import f16_close
from soc_real_time_renderer_amd import _abi, raster
from test_gpu_draws import DEV, SIZES, device_scene, gbuffer_images, host, materials, resolve_draws  # noqa: F401

pytestmark = pytest.mark.gpu
IMAGES = ("depth",) + D.GB_KEYS


def resolve_motion(g, ds, prev, materials, vis, out):
    raster.gbuffer_resolve_draws_motion(g, ds, prev, materials["table"], materials["count"], vis, out["depth"],
                                        out["albedo"], out["emissive"], out["normal"], out["velocity"])


def visibility(g, ds, W, H):
    vis = torch.zeros((H, W), dtype=torch.int64, device=DEV)
    raster.raster_visibility_draws(ds, np.ctypeslib.as_array(g.camera_projection_view_matrix), raster.CULL_FRONT, vis)
    return vis


@pytest.mark.parametrize("W,H", SIZES)
def test_previous_equal_to_current_reproduces_the_existing_resolve(soc, oracle, materials, W, H):
    """With the previous array aliasing the scene's transforms, and with a separate equal copy: all five images equal
    soc_gbuffer_resolve_draws' bit for bit."""
    c = MO.case(oracle, W, H)
    g, ds = c["g"], device_scene(c["scene"])
    vis = visibility(g, ds, W, H)
    want = gbuffer_images(W, H)
    resolve_draws(g, ds, materials, vis, want)
    assert (want["velocity"][..., :2] != 0).float().mean() > 0.2
    for prev in (ds.transforms, ds.transforms.clone()):
        got = gbuffer_images(W, H)
        resolve_motion(g, ds, prev, materials, vis, got)
        for k in IMAGES:
            assert torch.equal(got[k], want[k]), (k, prev is ds.transforms)


@pytest.mark.parametrize("W,H", SIZES)
def test_moved_entity_against_the_motion_oracle(soc, oracle, materials, W, H):
    """previous = entities_for(0.0), current = entities_for(0.35): the velocity follows the oracle; depth, albedo,
    emissive and normal are the non-motion call's; so is the velocity of every draw whose transform did not change."""
    c = MO.case(oracle, W, H)
    g, ds = c["g"], device_scene(c["scene"])
    prev = raster.transforms_device(*c["previous"], device=DEV)
    vis = visibility(g, ds, W, H)
    assert np.array_equal(host(vis).view(np.uint64), c["visibility"])
    plain, got = gbuffer_images(W, H), gbuffer_images(W, H)
    resolve_draws(g, ds, materials, vis, plain)
    resolve_motion(g, ds, prev, materials, vis, got)
    frac = f16_close(host(got["velocity"]), c["velocity"]).mean()
    print(f"{W}x{H} velocity: within tolerance on {frac:.6f}")
    assert frac >= 0.9999, (W, H, frac)
    for k in ("depth", "albedo", "emissive", "normal"):
        assert torch.equal(got[k], plain[k]), k
    moving = torch.from_numpy(np.isin(c["draw"], MO.moving_draws(c["scene"]))).to(DEV)
    assert moving.sum() >= 50 and (~moving).sum() >= 50
    assert torch.equal(got["velocity"][~moving], plain["velocity"][~moving])
    assert (got["velocity"][moving] != plain["velocity"][moving]).any(-1).float().mean() > 0.5


def test_render_graph_keeps_the_history(soc, oracle, materials):
    """Three frames with set_draw_motion, entity 1 moved before frames 1 and 2: frame 0 has the reference's velocity;
    frames 1 and 2 the direct motion entry point's given the preceding frame's transforms; the history array then holds
    frame 2's transforms; set_draw_motion(None) brings the reference's velocity back."""
    W, H = 160, 90
    phases = (0.0, 0.35, 0.5)
    g0 = D.frame_globals(W, H, 0)
    scenes = [D.with_transforms(D.build_scene(), g0, ph) for ph in phases]
    gs = [D.frame_globals(W, H, f) for f in (0, 1, 1)]
    ds = device_scene(scenes[0])
    history = torch.full_like(ds.transforms, float("nan"))            # whatever it holds, frame 0 does not read it
    vis_on, vis_off = (torch.zeros((H, W), dtype=torch.int64, device=DEV) for _ in range(2))
    fr_on, fr_off = soc.alloc_frame(W, H, DEV), soc.alloc_frame(W, H, DEV)
    off_scene = device_scene(scenes[0])
    on, off = soc.Renderer(fr_on), soc.Renderer(fr_off)
    on.set_draw_scene(ds, materials["table"], materials["count"], vis_on, shadow=False, motion=history)
    off.set_draw_scene(off_scene, materials["table"], materials["count"], vis_off, shadow=False)
    assert on.pass_names() == off.pass_names()
    alone = device_scene(scenes[0])                                    # the direct calls' scene, transforms rewritten per frame
    for f, (sc, g) in enumerate(zip(scenes, gs)):
        m, n = sc["transforms"]
        for scene in (ds, off_scene, alone):
            raster.update_transforms(scene.transforms, m, n)
        on.execute(g)
        off.execute(g)
        torch.cuda.synchronize()
        if f == 0:
            assert torch.equal(fr_on["velocity"], fr_off["velocity"])
        else:
            prev = raster.transforms_device(*scenes[f - 1]["transforms"], device=DEV)
            exp = gbuffer_images(W, H)
            resolve_motion(g, alone, prev, materials, visibility(g, alone, W, H), exp)
            torch.cuda.synchronize()
            assert torch.equal(fr_on["velocity"], exp["velocity"]), f
            assert not torch.equal(fr_on["velocity"], fr_off["velocity"]), f
        for k in ("depth", "albedo", "emissive", "normal"):
            assert torch.equal(fr_on[k], fr_off[k]), (f, k)
        assert torch.equal(history, ds.transforms), f                  # current -> previous, ready for the next frame
    assert torch.equal(history, raster.transforms_device(*scenes[2]["transforms"], device=DEV))
    on.set_draw_motion(None)
    on.execute(gs[2])
    off.execute(gs[2])
    torch.cuda.synchronize()
    assert torch.equal(fr_on["velocity"], fr_off["velocity"])
    on.close()
    off.close()


def test_null_previous_is_an_error_with_nothing_launched(soc, oracle, materials):
    W, H = 97, 55
    c = MO.case(oracle, W, H)
    ds = device_scene(c["scene"])
    vis = visibility(c["g"], ds, W, H)
    out = gbuffer_images(W, H)
    for t in out.values():
        t.fill_(0.25)
    with pytest.raises(soc.SocError, match="soc_gbuffer_resolve_draws_motion.*previous_transforms") as e:
        resolve_motion(c["g"], ds, None, materials, vis, out)
    assert e.value.rc == _abi.SOC_E_INVALID_ARG
    # the existing call's refusal of a workspace that was never built, under the new name
    unbuilt = device_scene(c["scene"], build=False)
    with pytest.raises(soc.SocError, match="soc_gbuffer_resolve_draws_motion.*not built"):
        resolve_motion(c["g"], unbuilt, ds.transforms, materials, vis, out)
    torch.cuda.synchronize()
    assert all((t == 0.25).all() for t in out.values())               # nothing was written
