"""The depth-of-field chain and pass on the GPU (soc_depth_of_field_mips, soc_depth_of_field, csrc/dof.hip) against the
float32 oracle (tests/dof_oracle.py), and as the opt-in pass pair of the render graph (Renderer.add_depth_of_field).

The chain is bit-exact: its arithmetic has no data-dependent choice. The pass chooses two levels and a blend factor per
pixel from lq, the lod in 1/256 steps, which ends a chain of float32 operations (depth -> object distance -> c -> rho ->
log2): a GPU pixel must equal, bit for bit, the oracle's pixel at lq_offset -1, 0 or +1 (no other value is accepted
anywhere), and at most 0.5 % of the geometry pixels may differ from lq_offset 0. That cap is a condition, not a
measurement: the kernel follows the oracle's operation order, so only a differently rounded operation can move lq;
evaluating the lod in float64 moves 0.6-1.2 % of these pixels (test_dof_oracle.py), a systematic error moves all."""
import json

import numpy as np
import pytest
import torch

import dof_inputs
import dof_oracle
import helpers
import views

pytestmark = pytest.mark.gpu
DEV = "cuda"
PARITY_CAP = 0.005
CHAIN_SIZES = dof_inputs.SIZES + [(5, 3)]


def _color(W, H):
    if (W, H) in dof_inputs.SIZES:
        return dof_inputs.images(W, H)[0]
    rng = np.random.default_rng(W * 100 + H)
    return rng.uniform(0.0, 4.0, (H, W, 4)).astype(np.float16)


def _oracle_levels(W, H):
    return dof_inputs.levels(W, H) if (W, H) in dof_inputs.SIZES else dof_oracle.chain(_color(W, H))


def _bits(t):
    return t.contiguous().view(torch.int16)


def _assert_chain(chain, want):
    got = chain.levels()
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert tuple(a.shape) == b.shape, k
        assert np.array_equal(a.cpu().contiguous().numpy().view(np.uint16), b.view(np.uint16)), f"level {k}"


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("W,H", CHAIN_SIZES)
def test_chain_bit_exact(soc, monkeypatch, W, H, fused):
    """Every level against the oracle, in the fused form (head + per-level + tail launches; 64x36 takes the head kernel,
    the odd extents the copy and the general blit) and the per-level form (SOC_DOF_CHAIN_FUSED=0)."""
    monkeypatch.setenv("SOC_DOF_CHAIN_FUSED", str(fused))
    soc.reload_tuning()
    color = torch.from_numpy(_color(W, H)).to(DEV)
    chain = soc.depth_of_field_chain(W, H, DEV)
    chain.buf.fill_(0x5B)
    soc.depth_of_field_mips(color, chain)
    torch.cuda.synchronize()
    _assert_chain(chain, _oracle_levels(W, H))


@pytest.mark.parametrize("W,H", [(512, 256), (259, 131)])
def test_chain_with_every_launch_kind(soc, W, H):
    """Extents whose level 2 (512x256: after the head kernel) or level 1 (259x131: after the copy, odd extents) is above
    the tail launch's 4096 texels: the head or copy, a per-level blit and the tail in one chain, several workgroups each."""
    rng = np.random.default_rng(5)
    c = rng.uniform(0.0, 4.0, (H, W, 4)).astype(np.float16)
    chain = soc.depth_of_field_chain(W, H, DEV)
    soc.depth_of_field_mips(torch.from_numpy(c).to(DEV), chain)
    torch.cuda.synchronize()
    _assert_chain(chain, dof_oracle.chain(c))


@pytest.mark.parametrize("layout", views.LAYOUTS)
@pytest.mark.parametrize("W,H", [(64, 36), (97, 55)])
def test_chain_on_padded_views(soc, W, H, layout):
    """A padded and offset colour view and a padded level 0 inside a poisoned allocation: the same levels, and every byte
    outside the written levels (level 0's row padding, the guards around the chain) untouched."""
    color, canvas = views.make_view(torch.from_numpy(_color(W, H)).to(DEV), layout, 0)
    pitch = 8 * (W + 3)
    n = int(soc.lib().soc_depth_of_field_chain_bytes(W, H, pitch))
    guard = 64
    alloc = torch.full((guard + n + guard,), 0x5B, dtype=torch.uint8, device=DEV)
    chain = soc.DepthOfFieldChain(alloc[guard:guard + n], W, H, pitch)
    soc.depth_of_field_mips(color, chain)
    torch.cuda.synchronize()
    _assert_chain(chain, _oracle_levels(W, H))
    assert (alloc[:guard] == 0x5B).all() and (alloc[guard + n:] == 0x5B).all()
    rows = chain.buf[:pitch * H].view(H, pitch)
    assert (rows[:, 8 * W:] == 0x5B).all()
    views.assert_padding_intact(canvas, H, W, layout, "color")      # an input: still its poison


def _device_inputs(soc, W, H):
    """(colour, depth, the chain built from the colour) of dof_inputs.images on the device."""
    color, depth = dof_inputs.images(W, H)
    color_t, depth_t = torch.from_numpy(color).to(DEV), torch.from_numpy(depth).to(DEV)
    chain = soc.depth_of_field_chain(W, H, DEV)
    soc.depth_of_field_mips(color_t, chain)
    return color_t, depth_t, chain


@pytest.mark.parametrize("gname", dof_inputs.GLOBALS)
@pytest.mark.parametrize("W,H", dof_inputs.SIZES)
def test_pass_parity_with_the_float32_oracle(soc, W, H, gname):
    g = dof_inputs.globals_set(gname, W, H)
    color_t, depth_t, chain = _device_inputs(soc, W, H)
    target = torch.full((H, W, 4), float("nan"), dtype=torch.float16, device=DEV)   # poisoned: every pixel is written
    soc.depth_of_field(g, depth_t, chain, target)
    torch.cuda.synchronize()
    share = dof_inputs.check_against_oracle(target.cpu().numpy(), W, H, gname)
    print(f"dof parity {W}x{H} {gname}: {share:.4%} of the geometry pixels differ from lq_offset 0")
    assert share <= PARITY_CAP
    # the target aliased to the colour the chain was built from (the reference's arrangement): the same bits
    soc.depth_of_field(g, depth_t, chain, color_t)
    torch.cuda.synchronize()
    assert torch.equal(_bits(color_t), _bits(target))


@pytest.mark.parametrize("layout", views.LAYOUTS)
def test_pass_on_padded_views(soc, layout):
    W, H = 97, 55
    g = dof_inputs.globals_set("focus20", W, H)
    _, depth_t, chain = _device_inputs(soc, W, H)
    tight = torch.zeros((H, W, 4), dtype=torch.float16, device=DEV)
    soc.depth_of_field(g, depth_t, chain, tight)
    depth_v, depth_c = views.make_view(depth_t, layout, 0)
    target_v, target_c = views.make_view(torch.zeros_like(tight), layout, 1, role="out")
    soc.depth_of_field(g, depth_v, chain, target_v)
    torch.cuda.synchronize()
    assert views.bits_equal(target_v, tight)
    views.assert_padding_intact(target_c, H, W, layout, "target")
    views.assert_padding_intact(depth_c, H, W, layout, "depth")


def _frame(soc, W, H, gb):
    fr = soc.alloc_frame(W, H, DEV)
    for k in ("albedo", "emissive", "normal", "velocity", "depth"):
        fr[k].copy_(torch.from_numpy(gb[k]))
    fr["shadow"] = torch.from_numpy(gb["shadow"]).to(DEV)
    fr["noise"].copy_(torch.from_numpy(gb["noise"]))
    return fr


def test_render_graph_passes(soc):
    """A 64x36 frame on an unfused-histogram renderer: the colour after the pair obeys the parity rule against the oracle
    applied to the colour of an identical renderer without it, the AutoExposure bins are those of the histogram pass run
    alone on that blurred colour, and the metrics record's "Depth Of Field" group is no longer 0."""
    W, H = 64, 36
    g, gb = helpers.cached_variant_inputs("default", W, H)
    with np.errstate(invalid="ignore"):
        assert 0.05 < (gb["depth"] < 1.0).mean()
    colors = {}
    for with_pass in (False, True):
        fr = _frame(soc, W, H, gb)
        r = soc.Renderer(fr, timing=True, fused_histogram=False)
        if with_pass:
            chain = soc.depth_of_field_chain(W, H, DEV)
            r.add_depth_of_field(chain)
        r.execute(g, soc.PHASE_PRE_EXPOSURE)
        torch.cuda.synchronize()
        colors[with_pass] = fr["color"].clone()
        if with_pass:
            alone = soc.auto_exposure_buffer(DEV)
            soc.generate_luminance_histogram(g, fr["color"], alone)
            torch.cuda.synchronize()
            assert torch.equal(fr["auto_exposure"][1:], alone[1:])
            assert int(alone[1:].sum()) == W * H
            groups = json.loads(r.metrics_json())["groups"]
            assert groups["Depth Of Field"] > 0.0
            _assert_chain(chain, dof_oracle.chain(colors[False].cpu().numpy()))
        r.execute(g, soc.PHASE_POST_EXPOSURE)
        torch.cuda.synchronize()
        r.close()
    plain = colors[False].cpu().numpy()
    share = dof_inputs.check_against_oracle(colors[True].cpu().numpy(), W, H, None, depth=gb["depth"],
                                            level_list=dof_oracle.chain(plain), g=g)
    print(f"dof frame parity: {share:.4%} of the geometry pixels differ from lq_offset 0")
    assert share <= PARITY_CAP
    assert not torch.equal(_bits(colors[True]), _bits(colors[False]))
