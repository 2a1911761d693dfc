"""The sky lane's book-keeping: static cloud tables built once per renderer (SOC_CLOUDS_STATIC_TABLES) and the counter
blocks alternating by frame.

Every image and the exposure must be the bits of the per-frame build. Two small extents break the
tilings: 200x72 (no multiple of 64 in either axis, a partial last 64x64 classify region, four regions across) and
66x34 (an odd pair column at the right edge). The depth images are crafted: a sky edge that cuts through pixel pairs,
a sky count that is no multiple of 256, a frame without sky followed by a frame of sky only."""
import numpy as np
import pytest
import torch

from helpers import globals_for, sponza_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
EXTENTS = [(200, 72), (66, 34)]
OFF = {"SOC_CLOUDS_STATIC_TABLES": "0"}

_INPUTS = {}


def _inputs(W, H):
    """The Sponza G-buffer at the extent (shared, never modified: callers copy what they change)."""
    if (W, H) not in _INPUTS:
        _INPUTS[(W, H)] = sponza_inputs(W, H, shadow_size=128, elapsed=10.0)
    return _INPUTS[(W, H)]


def _frame(soc, W, H, gb):
    fr = soc.alloc_frame(W, H, DEV)
    for k in ("albedo", "emissive", "normal", "velocity", "depth"):
        fr[k].copy_(torch.from_numpy(gb[k]))
    fr["shadow"] = torch.from_numpy(gb["shadow"]).to(DEV)
    fr["noise"].copy_(torch.from_numpy(gb["noise"]))
    return fr


def _edge_depth(W, H, gb, k):
    """The G-buffer's depth kept below 1, with sky (1.0f) right of a slanted edge x + 0.37 y > c_k: the edge crosses
    pixel pairs at odd and even columns."""
    d = np.minimum(gb["depth"], np.float32(0.9990234)).astype(np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    d[(xx + 0.37 * yy) > (0.30 + 0.09 * k) * W] = 1.0
    return d


def _sequence_depths(W, H, gb):
    ds = [_edge_depth(W, H, gb, k) for k in range(6)]
    ds[3] = np.minimum(gb["depth"], np.float32(0.9990234)).astype(np.float32)   # no sky pixel at all
    ds[4] = np.ones((H, W), np.float32)                                          # sky only
    for k in (0, 1, 2, 5):
        n = int((ds[k] == 1.0).sum())
        assert n > 0 and n % 256 != 0, (k, n)
    assert not (ds[3] == 1.0).any()
    return ds


def _globals_seq(W, H, n=6):
    """Camera position and elapsed time change every frame."""
    return [globals_for(W, H, frames=2 + k, elapsed=10.0 + 3.7 * k, move=0.21) for k in range(n)]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16) if a.dtype == np.float16 else a


def _snapshot(soc, fr, r):
    torch.cuda.synchronize()
    return {"clouds": fr["clouds"].cpu().numpy(), "color": _bits(fr["color"].cpu().numpy()),
            "output": fr["output"].cpu().numpy(), "resolved": _bits(r.resolved().cpu().numpy()),
            "exposure": np.float32(soc.exposure_of(fr["auto_exposure"])).view(np.uint32)}


def _render(soc, r, fr, g, split):
    """One frame; split: the two-phase frame, whose folded pre-resolve histogram is read between the calls."""
    if not split:
        r.execute(g)
        return _snapshot(soc, fr, r)
    r.execute(g, soc.PHASE_PRE_EXPOSURE)
    torch.cuda.synchronize()
    hist = fr["auto_exposure"].cpu().numpy().copy()
    r.execute(g, soc.PHASE_POST_EXPOSURE)
    s = _snapshot(soc, fr, r)
    s["histogram"] = hist
    return s


def _set_knobs(soc, monkeypatch, env):
    for k in list(OFF) + ["SOC_CLOUDS_OD_LUT", "SOC_CLOUDS_NOISE_TABLE", "SOC_CLOUDS_SKY_TABLE"]:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    soc.reload_tuning()


def _run_sequence(soc, monkeypatch, env, W, H, depths, gs, split, **renderer_kw):
    _set_knobs(soc, monkeypatch, env)
    g0, gb = _inputs(W, H)
    fr = _frame(soc, W, H, gb)
    r = soc.Renderer(fr, **renderer_kw)
    out = []
    for d, g in zip(depths, gs):
        torch.cuda.synchronize()
        fr["depth"].copy_(torch.from_numpy(d))
        torch.cuda.synchronize()
        out.append(_render(soc, r, fr, g, split))
    r.close()
    return out


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{what}: {k} differs on {int((np.asarray(a[k]) != np.asarray(b[k])).sum())} values"


@pytest.mark.parametrize("split", [False, True], ids=["one_call", "two_phase"])
@pytest.mark.parametrize("W,H", EXTENTS)
def test_sequence_identical_to_per_frame_build(soc, monkeypatch, W, H, split):
    """Six consecutive frames on one renderer with the static tables (the default at these extents), against the same
    frames with the knob off."""
    _, gb = _inputs(W, H)
    depths, gs = _sequence_depths(W, H, gb), _globals_seq(W, H)
    new = _run_sequence(soc, monkeypatch, {}, W, H, depths, gs, split)
    old = _run_sequence(soc, monkeypatch, OFF, W, H, depths, gs, split)
    for k, (a, b) in enumerate(zip(new, old)):
        _assert_same(a, b, f"frame {k}")
    # a static-inputs renderer (CloudRendering ahead of the fork), one without the sky lane, and a high-priority sky
    # lane (the hoisted classification)
    for kw in ({"static_inputs": True}, {"sky_lane": False}, {"sky_lane_queue": "high"}):
        part = _run_sequence(soc, monkeypatch, {}, W, H, depths, gs, split, **kw)
        for k, (a, b) in enumerate(zip(part, old)):
            _assert_same(a, b, f"{kw} frame {k}")
    # the existing knobs keep working with the static tables: each table off gives the bits of the per-frame build
    # with that table off
    for knob in ("SOC_CLOUDS_OD_LUT", "SOC_CLOUDS_NOISE_TABLE", "SOC_CLOUDS_SKY_TABLE"):
        a_seq = _run_sequence(soc, monkeypatch, {knob: "0"}, W, H, depths[:3], gs[:3], split)
        b_seq = _run_sequence(soc, monkeypatch, dict(OFF, **{knob: "0"}), W, H, depths[:3], gs[:3], split)
        for k, (a, b) in enumerate(zip(a_seq, b_seq)):
            _assert_same(a, b, f"{knob}=0 frame {k}")


def _c2_bits(g):
    s = np.array([-float(v) for v in g.sun_info.direction], np.float32)
    return np.float32(np.float32(s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]).view(np.uint32)


def test_sun_change_and_noise_invalidation(soc, monkeypatch):
    """The sun direction changes between frames 2 and 3 (a new bit pattern of C2); the noise image is rewritten in
    place before frame 4 and the tables are invalidated. Every frame equals a freshly created renderer's."""
    W, H = EXTENTS[0]
    _set_knobs(soc, monkeypatch, {})
    _, gb = _inputs(W, H)
    depths, gs = _sequence_depths(W, H, gb), _globals_seq(W, H)
    sun0 = [float(v) for v in gs[0].sun_info.direction]
    sun1 = None
    for scale in (0.75, 0.5, 1.5):   # a direction of another length: dot(sun, sun) cannot keep its bits
        cand = [v * scale for v in sun0]
        g = gs[3]
        g.sun_info.direction[:] = cand
        if _c2_bits(g) != _c2_bits(gs[0]):
            sun1 = cand
            break
    assert sun1 is not None
    for k in (3, 4, 5):
        gs[k].sun_info.direction[:] = sun1
    noise1 = np.ascontiguousarray(np.roll(gb["noise"], (5, 11), axis=(0, 1))[::-1])
    assert not np.array_equal(noise1, gb["noise"])
    noises = [gb["noise"]] * 4 + [noise1] * 2

    fr = _frame(soc, W, H, gb)
    r = soc.Renderer(fr)
    fr_stale = _frame(soc, W, H, gb)      # the same frames without the invalidation: what the call is for
    r_stale = soc.Renderer(fr_stale)
    for k in range(6):
        torch.cuda.synchronize()
        for f in (fr, fr_stale):
            f["depth"].copy_(torch.from_numpy(depths[k]))
            if k == 4:
                f["noise"].copy_(torch.from_numpy(noise1))   # the same allocation: only the invalidation tells
        if k == 4:
            r.invalidate_cloud_tables()
        torch.cuda.synchronize()
        r.execute(gs[k])
        r_stale.execute(gs[k])
        torch.cuda.synchronize()
        # the colour where SkyCompose writes it (elsewhere it carries the bloom the chain accumulates in the emissive image)
        sky = depths[k] == 1.0
        got = {"clouds": fr["clouds"].cpu().numpy(), "sky_color": _bits(fr["color"].cpu().numpy())[sky]}
        gb_k = dict(gb, depth=depths[k], noise=noises[k])
        fr2 = _frame(soc, W, H, gb_k)
        r2 = soc.Renderer(fr2)
        r2.execute(gs[k])
        torch.cuda.synchronize()
        want = {"clouds": fr2["clouds"].cpu().numpy(), "sky_color": _bits(fr2["color"].cpu().numpy())[sky]}
        r2.close()
        _assert_same(got, want, f"frame {k}")
        if k == 4:   # the rewritten texels reach the image only through the rebuilt tables
            assert not np.array_equal(fr_stale["clouds"].cpu().numpy(), want["clouds"])
    r.close()
    r_stale.close()


def test_standalone_entry_stays_stateless(soc, monkeypatch):
    """soc_cloud_rendering twice on one workspace with different noise contents in the same image: each call gives
    the result of a call on a fresh workspace."""
    W, H = EXTENTS[0]
    _set_knobs(soc, monkeypatch, {})
    g, gb = _inputs(W, H)
    d = _edge_depth(W, H, gb, 1)
    noise1 = np.ascontiguousarray(gb["noise"][::-1, ::-1])
    depth = torch.from_numpy(d).to(DEV)
    noise = torch.from_numpy(gb["noise"]).to(DEV)
    ws = soc.cloud_rendering_workspace(W, H, DEV)
    got, want = [], []
    for nz in (gb["noise"], noise1):
        noise.copy_(torch.from_numpy(nz))
        torch.cuda.synchronize()
        o = torch.zeros(H, W, 4, dtype=torch.uint8, device=DEV)
        soc.cloud_rendering(g, depth, noise, o, ws)
        torch.cuda.synchronize()
        got.append(o.cpu().numpy())
        o2 = torch.zeros(H, W, 4, dtype=torch.uint8, device=DEV)
        soc.cloud_rendering(g, depth, noise, o2, soc.cloud_rendering_workspace(W, H, DEV))
        torch.cuda.synchronize()
        want.append(o2.cpu().numpy())
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert not np.array_equal(got[0], got[1])   # the noise does reach the image
