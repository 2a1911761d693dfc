"""SOC_BLOOM_ZERO_SKIP (-m gpu): the weighted bloom chain's first and last kernels skip their filters on tiles / rows
whose input has the bit pattern 0x0000 in every RGB half and store pack3(+0, +0, +0) there. With the knob 0 every tile
is filtered; both forms must give the same bits in mip1 (after the upsweep), mip3 and the chain's output.

136 x 40: every tile touches an image edge (the clamped per-entry path). 968 x 552: interior register-run tiles; the
mip1 width 484 is no multiple of 30 and the output width no multiple of 62 (partial last tile column / strip)."""
import numpy as np
import pytest
import torch

from helpers import globals_for, random_rgba16

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIZES = [(136, 40), (968, 552)]
ONE = np.float16(1.0).view(np.uint16)


def zeros_u16(H, W):
    """RGB 0x0000, alpha 1.0, as uint16 bit patterns."""
    a = np.zeros((H, W, 4), np.uint16)
    a[..., 3] = ONE
    return a


def chain_both(soc, monkeypatch, W, H, images):
    """[(knob-off, knob-on)] per image, each (mip1, mip3, out) of soc.bloom_weighted_stage(..., 0)."""
    g = globals_for(W, H)
    shapes = [(H >> i, W >> i, 4) for i in range(4)]
    ems = [torch.from_numpy(np.ascontiguousarray(a).view(np.float16)).to(DEV) for a in images]
    res = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("SOC_BLOOM_ZERO_SKIP", knob)
        soc.reload_tuning()
        res[knob] = []
        for em in ems:
            mips = [torch.full(sh, 3.0, dtype=torch.float16, device=DEV) for sh in shapes]
            out = torch.full_like(em, 3.0)
            soc.bloom_weighted_stage(g, em, mips, out, 0)
            res[knob].append((mips[1], mips[3], out))
    torch.cuda.synchronize()
    monkeypatch.delenv("SOC_BLOOM_ZERO_SKIP")
    soc.reload_tuning()
    return list(zip(res["0"], res["1"]))


def bits(t):
    return t.view(torch.int16)


def assert_same(pairs, labels):
    for (off, on), label in zip(pairs, labels):
        for name, a, b in zip(("mip1", "mip3", "out"), off, on):
            # bit patterns, so that NaN == NaN and -0 != +0
            assert torch.equal(bits(a), bits(b)), (label, name, (bits(a) != bits(b)).float().mean().item())


@pytest.mark.parametrize("W,H", SIZES)
def test_all_zero_is_exactly_zero(soc, monkeypatch, W, H):
    """All RGB 0x0000 with alpha 1.0 and with random alpha: the same bits either way, and mip1 and the output are exactly
    (+0, +0, +0, 1.0)."""
    a1 = zeros_u16(H, W)
    ar = zeros_u16(H, W)
    ar[..., 3] = random_rgba16(H, W, seed=5, alpha=None).view(np.uint16)[..., 3]
    pairs = chain_both(soc, monkeypatch, W, H, [a1, ar])
    assert_same(pairs, ["alpha 1", "random alpha"])
    for off, on in pairs:
        for t in (on[0], on[2], off[0], off[2]):
            u = t.cpu().numpy().view(np.uint16)
            assert (u[..., :3] == 0).all() and (u[..., 3] == ONE).all()


def lit_positions(W, H):
    pos = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 2)]
    # either side of a first-kernel tile edge (60 x 16 texels) and of the edge of its +-4 halo
    pos += [(x, y) for x in (55, 56, 59, 60, 63, 64) for y in (11, 12, 15, 16, 19, 20)]
    # the last kernel's strip edges (62 x 16 outputs)
    pos += [(x, y) for x in (61, 62, 123, 124) for y in (15, 16, 31, 32)]
    return pos


@pytest.mark.parametrize("W,H", SIZES)
def test_one_lit_texel(soc, monkeypatch, W, H):
    """One texel of 8.0 in a zero image, at the corners, the centre and either side of the tile, halo and strip edges: a
    neighbouring tile's vote must see a lit texel in its halo."""
    pos = lit_positions(W, H)
    images = []
    for x, y in pos:
        a = zeros_u16(H, W)
        a[y, x, :3] = np.float16(8.0).view(np.uint16)
        images.append(a)
    pairs = chain_both(soc, monkeypatch, W, H, images)
    assert_same(pairs, pos)
    for (off, on), p in zip(pairs, pos):
        assert (on[2][..., :3] != 0).any(), p   # the lit texel reaches the output


@pytest.mark.parametrize("W,H", SIZES)
def test_special_values(soc, monkeypatch, W, H):
    """-0 everywhere (0x8000: not covered by the +0 argument, so it must not be skipped, or must give the same bits), and
    one texel of NaN, +Inf and the smallest subnormal (0x0001) in a zero image: non-zero bit patterns, the full path."""
    neg = zeros_u16(H, W)
    neg[..., :3] = 0x8000
    images, labels = [neg], ["-0"]
    for label, v in (("nan", 0x7E00), ("inf", 0x7C00), ("subnormal", 0x0001)):
        for x, y in ((W // 2, H // 2), (60, 16), (W - 1, H - 1)):
            a = zeros_u16(H, W)
            a[y, x, :3] = v
            images.append(a)
            labels.append((label, x, y))
    assert_same(chain_both(soc, monkeypatch, W, H, images), labels)


@pytest.mark.parametrize("W,H", SIZES)
def test_dense_and_band(soc, monkeypatch, W, H):
    """Dense random emissive (no tile is skipped), and lit texels confined to one horizontal band (skipped and filtered
    tiles in one launch, and tiles that change between the two from one persistent-loop step to the next)."""
    dense = random_rgba16(H, W, seed=43, hi=16.0).view(np.uint16)
    band = zeros_u16(H, W)
    y0, y1 = (200, 261) if H > 261 else (H // 2 - 3, H // 2 + 4)
    band[y0:y1, :, :3] = dense[y0:y1, :, :3]
    sparse = zeros_u16(H, W)   # scattered lit texels inside the band
    m = np.random.default_rng(7).random((y1 - y0, W)) < 0.002
    sparse[y0:y1][m] = dense[y0:y1][m]
    assert_same(chain_both(soc, monkeypatch, W, H, [dense, band, sparse]), ["dense", "band", "sparse band"])


def test_frame_with_bloom_in_composition(soc, monkeypatch):
    """The bloom's last stage inside Composition (Up10Tile, a high-priority sky lane: in-kernel from the second frame on):
    an all-zero mip1 tile takes the constant instead of the tile's sums. With an all-zero emissive image and with one lit
    texel, three frames' composition colour has the same bits with the knob 0 and 1."""
    import ctypes as C

    from helpers import sponza_inputs
    W, H = 200, 120
    _g0, gb = sponza_inputs(W, H, elapsed=10.0)
    zero = zeros_u16(H, W)
    lit = zeros_u16(H, W)
    lit[61, 97, :3] = np.float16(8.0).view(np.uint16)
    for label, emis in (("zero", zero), ("lit", lit)):
        seqs = []
        for knob in ("0", "1"):
            monkeypatch.setenv("SOC_BLOOM_ZERO_SKIP", knob)
            soc.reload_tuning()
            fr = soc.alloc_frame(W, H, DEV, bloom_output=True)
            for k in ("albedo", "normal", "velocity", "depth"):
                fr[k].copy_(torch.from_numpy(gb[k]))
            fr["emissive"].copy_(torch.from_numpy(emis.view(np.float16)))
            fr["shadow"] = torch.from_numpy(np.ascontiguousarray(gb["shadow"])).to(DEV)
            fr["noise"].copy_(torch.from_numpy(gb["noise"]))
            r = soc.Renderer(fr, static_inputs=True, bloom_in_composition=True, sky_lane_queue="high")
            cam = soc.make_camera((-14.0, 2.2, 0.3), (0.0, -0.42, 0.0))
            ji = C.c_uint32(0)
            g = soc.globals_defaults(W, H)
            seq = []
            for f in range(3):
                soc.frame_update(g, cam, W, H, 0.016, ji)
                cam.position[0] += 0.05
                r.execute(g)
                seq.append(fr["color"].clone())
                if f == 0:
                    fr["bloom_output"].fill_(7.0)
            torch.cuda.synchronize()
            assert bool((fr["bloom_output"] == 7.0).all()), "the in-Composition path was not taken"
            seqs.append(seq)
            r.close()
        monkeypatch.delenv("SOC_BLOOM_ZERO_SKIP")
        soc.reload_tuning()
        for f, (a, b) in enumerate(zip(*seqs)):
            assert torch.equal(bits(a), bits(b)), (label, f)
