"""SOC_BLOOM_SPARSE (-m gpu): under SOC_RENDERER_BLOOM_IN_COMPOSITION beside a low-priority sky lane, the weighted
chain's last stage (bloomw_up10r) leaves the strips unwritten whose 32 x 16 cells are all proven zero from mip3, and
Composition, the bloom output's only reader, proves the same cells and takes pack3(+0, +0, +0) there instead of
loading them. Against the same renderer with SOC_BLOOM_SPARSE=0 (every pixel written and loaded), compared as bit
patterns; the bloom output is pre-filled with a 7.0 sentinel, so an unwritten pixel shows.

192 x 64: 6 x 4 cells, 4 strips per strip row. 200 x 72: a partial last cell row and column and a partial strip, mip3
25 x 9. 968 x 552 (one-lit and dense only): many strips, the output width no multiple of 62 or 32."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import random_rgba16, sponza_inputs
from views import assert_padding_intact, make_view

pytestmark = pytest.mark.gpu

DEV = "cuda"
SMALL = [(192, 64), (200, 72)]
LARGE = (968, 552)
ONE = int(np.float16(1.0).view(np.uint16))
SENTINEL = 7.0
CW, CH = 32, 16

_INPUTS = {}


def inputs(W, H):
    if (W, H) not in _INPUTS:
        _INPUTS[(W, H)] = sponza_inputs(W, H, elapsed=10.0)
    return _INPUTS[(W, H)]


def zeros_u16(H, W):
    """RGB 0x0000, alpha 1.0, as uint16 bit patterns."""
    a = np.zeros((H, W, 4), np.uint16)
    a[..., 3] = ONE
    return a


def lit_u16(H, W, x, y, bits=None):
    a = zeros_u16(H, W)
    a[y, x, :3] = int(np.float16(8.0).view(np.uint16)) if bits is None else bits
    return a


def bits(t):
    if t.dtype == torch.float16:
        return t.contiguous().view(torch.int16)
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32)
    return t.contiguous()


def same(a, b):
    return torch.equal(bits(a), bits(b))


def run(soc, monkeypatch, knob, W, H, emissives, lane="low", lights=False, refill=True, generic=(), layout=None, **kw):
    """One renderer, one frame per emissive image (uint16 bit patterns). Returns ([per-frame {color, output, bloom}],
    {resolved, auto_exposure}). refill: the sentinel before every frame, else before the first only.
    generic: the frames whose globals resolution is W - 2 (Composition's generic path). layout: mip3 and the bloom
    output as padded, offset views (views.make_view)."""
    monkeypatch.setenv("SOC_BLOOM_SPARSE", knob)
    soc.reload_tuning()
    g, gb = inputs(W, H)
    fr = soc.alloc_frame(W, H, DEV, bloom_output=True)
    for k in ("albedo", "normal", "velocity", "depth"):
        fr[k].copy_(torch.from_numpy(gb[k]))
    fr["shadow"] = torch.from_numpy(np.ascontiguousarray(gb["shadow"])).to(DEV)
    fr["noise"].copy_(torch.from_numpy(gb["noise"]))
    canvases = []
    if layout:
        fr["bloom_mips"][3], c3 = make_view(fr["bloom_mips"][3], layout[0], 1, "out")
        fr["bloom_output"], co = make_view(fr["bloom_output"], layout[1], 0, "out")
        canvases = [("mip3", fr["bloom_mips"][3], c3, layout[0]), ("bloom_output", fr["bloom_output"], co, layout[1])]
    fr["bloom_output"].fill_(SENTINEL)
    r = soc.Renderer(fr, bloom_in_composition=True, sky_lane_queue=lane, **kw)
    gf = type(g)()
    C.pointer(gf)[0] = g
    if lights:
        import bench
        soc.scene_update(gf, bench.point_lights_c3b())
    gg = type(g)()
    C.pointer(gg)[0] = gf
    gg.resolution[0] = W - 2
    seq = []
    for f, em in enumerate(emissives):
        fr["emissive"].copy_(torch.from_numpy(np.ascontiguousarray(em).view(np.float16)))
        if refill and f:
            fr["bloom_output"].fill_(SENTINEL)
        r.execute(gg if f in generic else gf)
        seq.append({"color": fr["color"].clone(), "output": fr["output"].clone(), "bloom": fr["bloom_output"].clone()})
    torch.cuda.synchronize()
    end = {"resolved": r.resolved().clone(), "auto_exposure": fr["auto_exposure"].clone()}
    for name, v, c, lay in canvases:
        assert_padding_intact(c, int(v.shape[0]), int(v.shape[1]), lay, name)
    r.close()
    monkeypatch.delenv("SOC_BLOOM_SPARSE")
    soc.reload_tuning()
    return seq, end


def both(soc, monkeypatch, *a, **kw):
    return run(soc, monkeypatch, "0", *a, **kw), run(soc, monkeypatch, "1", *a, **kw)


def assert_frames_identical(dense, sparse, labels, keys=("color", "output")):
    (dseq, dend), (sseq, send) = dense, sparse
    for d, s, label in zip(dseq, sseq, labels):
        for k in keys:
            assert same(d[k], s[k]), (label, k, (bits(d[k]) != bits(s[k])).float().mean().item())
    for k in dend:
        assert same(dend[k], send[k]), k


def sentinel_mask(bloom):
    """(H, W) bool: the pixel still holds the sentinel in all four halves."""
    return (bloom == SENTINEL).all(dim=2).cpu().numpy()


def cells(mask):
    """{(a, b): the cell's (H, W) slice} of a 32 x 16 tiling."""
    H, W = mask.shape
    return {(a, b): (slice(b * CH, min(b * CH + CH, H)), slice(a * CW, min(a * CW + CW, W)))
            for b in range(-(-H // CH)) for a in range(-(-W // CW))}


def check_cells(dense_bloom, sparse_bloom, label):
    """A cell that holds any sentinel is a proven one: the dense output there is all (+0, +0, +0, 1), in its written
    pixels too. A strip (62 columns) stores all of its pixels or none and is up to three cells wide, so a proven cell
    beside an unproven one holds a written strip's columns next to an untouched strip's: what is left of the sentinel
    in a cell is whole columns of it, changing only at strip edges. Every other cell equals the dense output bit for
    bit. Returns (cells with sentinel, cells written whole)."""
    m = sentinel_mask(sparse_bloom)
    d = dense_bloom.cpu().numpy().view(np.uint16)
    s = sparse_bloom.cpu().numpy().view(np.uint16)
    assert not sentinel_mask(dense_bloom).any(), label
    n_sent = n_written = 0
    for ab, (ys, xs) in cells(m).items():
        if m[ys, xs].any():
            assert (d[ys, xs, :3] == 0).all() and (d[ys, xs, 3] == ONE).all(), (label, ab, "dense is not zero there")
            cols = m[ys, xs].all(axis=0)
            assert (m[ys, xs].any(axis=0) == cols).all(), (label, ab, "a column partly written")
            edges = np.nonzero(cols[1:] != cols[:-1])[0] + 1 + xs.start
            assert all(int(e) % 62 == 0 for e in edges), (label, ab, "written columns do not end at a strip edge", edges)
            w = ~m[ys, xs]
            assert (d[ys, xs][w] == s[ys, xs][w]).all(), (label, ab, "a written pixel differs from the dense output")
            n_sent += 1
        else:
            assert (d[ys, xs] == s[ys, xs]).all(), (label, ab, "differs from the dense output")
            n_written += 1
    return n_sent, n_written


@pytest.mark.parametrize("W,H", SMALL)
def test_all_zero_emissive_writes_nothing(soc, monkeypatch, W, H):
    """All-zero emissive with alpha 1 and with random alpha: every bloom-output pixel still holds the sentinel; colour,
    framebuffer, resolved history and exposure are those of the dense run."""
    ar = zeros_u16(H, W)
    ar[..., 3] = random_rgba16(H, W, seed=5, alpha=None).view(np.uint16)[..., 3]
    dense, sparse = both(soc, monkeypatch, W, H, [zeros_u16(H, W), ar])
    assert_frames_identical(dense, sparse, ["alpha 1", "random alpha"])
    for f in sparse[0]:
        assert sentinel_mask(f["bloom"]).all()
    for f in dense[0]:
        assert not sentinel_mask(f["bloom"]).any()


def lit_positions(W, H):
    pos = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 2)]
    pos += [(x, y) for x in (31, 32) for y in (15, 16)]                    # either side of a cell edge
    pos += [(x, y) for x in (61, 62, 123, 124) for y in (15, 16)]          # either side of a strip edge
    return pos


@pytest.mark.parametrize("W,H", SMALL + [LARGE])
def test_one_lit_texel(soc, monkeypatch, W, H):
    """One texel of 8.0 in a zero image, one frame per position: colour identical to dense; a cell with sentinel left
    in it is zero in the dense output, every other cell carries the dense bits (check_cells); both kinds exist."""
    pos = lit_positions(W, H)
    dense, sparse = both(soc, monkeypatch, W, H, [lit_u16(H, W, x, y) for x, y in pos])
    assert_frames_identical(dense, sparse, pos)
    for d, s, p in zip(dense[0], sparse[0], pos):
        n_sent, n_written = check_cells(d["bloom"], s["bloom"], p)
        print(f"{W}x{H} lit {p}: {n_sent} cells untouched, {n_written} written")
        assert n_sent > 0 and n_written > 0, (p, n_sent, n_written)
        assert (s["bloom"][..., :3][~torch.from_numpy(sentinel_mask(s["bloom"])).to(DEV)] != 0).any(), p


@pytest.mark.parametrize("W,H", SMALL)
def test_special_values(soc, monkeypatch, W, H):
    """-0 everywhere, and one texel of NaN, +Inf and the smallest subnormal (0x0001): bit patterns the +0 argument does
    not cover. Identical to dense; written cells carry the dense bits."""
    neg = zeros_u16(H, W)
    neg[..., :3] = 0x8000
    images, labels = [neg], ["-0"]
    for label, v in (("nan", 0x7E00), ("inf", 0x7C00), ("subnormal", 0x0001)):
        for x, y in ((W // 2, H // 2), (62, 16)):
            images.append(lit_u16(H, W, x, y, v))
            labels.append((label, x, y))
    dense, sparse = both(soc, monkeypatch, W, H, images)
    assert_frames_identical(dense, sparse, labels)
    for d, s, label in zip(dense[0], sparse[0], labels):
        check_cells(d["bloom"], s["bloom"], label)


@pytest.mark.parametrize("W,H", SMALL + [LARGE])
def test_dense_emissive(soc, monkeypatch, W, H):
    """Dense random emissive: nothing is proven, no sentinel is left, everything identical to dense."""
    em = random_rgba16(H, W, seed=43, hi=16.0).view(np.uint16)
    dense, sparse = both(soc, monkeypatch, W, H, [em])
    assert_frames_identical(dense, sparse, ["dense"], keys=("color", "output", "bloom"))
    assert not sentinel_mask(sparse[0][0]["bloom"]).any()


@pytest.mark.parametrize("W,H", SMALL)
def test_three_frames_without_refill(soc, monkeypatch, W, H):
    """Lit at A, then all zero, then lit at B in another cell, on one renderer, the bloom output never refilled: the cells
    around A hold frame 1's values through frames 2 and 3 where the last stage no longer writes them, and Composition
    must not read them. Each frame's colour identical to dense."""
    A, B = (40, 20), (W - 20, H - 10)
    images = [lit_u16(H, W, *A), zeros_u16(H, W), lit_u16(H, W, *B)]
    dense, sparse = both(soc, monkeypatch, W, H, images, refill=False)
    assert_frames_identical(dense, sparse, ["lit A", "zero", "lit B"])
    a = (slice(A[1] // CH * CH, A[1] // CH * CH + CH), slice(A[0] // CW * CW, A[0] // CW * CW + CW))
    stale = sparse[0][1]["bloom"][a]
    assert same(stale, sparse[0][0]["bloom"][a]) and (stale[..., :3] != 0).any()   # frame 1's values, left in place


@pytest.mark.parametrize("W,H", SMALL)
def test_generic_path_frame_writes_everything(soc, monkeypatch, W, H):
    """A frame whose globals resolution is W - 2 takes Composition's generic path, which reads every pixel of the bloom
    output: no sentinel is left although the emissive is zero; the matching frame after it is sparse again."""
    z = zeros_u16(H, W)
    dense, sparse = both(soc, monkeypatch, W, H, [z, z, z], generic=(1,), sky_split=False)
    assert_frames_identical(dense, sparse, ["pair", "generic", "pair"])
    assert sentinel_mask(sparse[0][0]["bloom"]).all()
    assert not sentinel_mask(sparse[0][1]["bloom"]).any()
    assert sentinel_mask(sparse[0][2]["bloom"]).all()


@pytest.mark.parametrize("W,H", SMALL)
def test_standalone_stage_4_stays_dense(soc, W, H):
    """soc_bloom_weighted_stage(4), the public entry, on zero mips: every output pixel written."""
    from helpers import globals_for
    g = globals_for(W, H)
    z = torch.from_numpy(zeros_u16(H, W).view(np.float16)).to(DEV)
    mips = [torch.from_numpy(zeros_u16(H >> i, W >> i).view(np.float16)).to(DEV) for i in range(4)]
    out = torch.full((H, W, 4), SENTINEL, dtype=torch.float16, device=DEV)
    soc.bloom_weighted_stage(g, z, mips, out, 4)
    torch.cuda.synchronize()
    assert not sentinel_mask(out).any()
    u = out.cpu().numpy().view(np.uint16)
    assert (u[..., :3] == 0).all() and (u[..., 3] == ONE).all()


def test_point_lights(soc, monkeypatch):
    """The lights kernel (the C3b point lights): zero, one lit texel and dense emissive identical to dense."""
    W, H = 200, 72
    images = [zeros_u16(H, W), lit_u16(H, W, 62, 16), random_rgba16(H, W, seed=44, hi=16.0).view(np.uint16)]
    dense, sparse = both(soc, monkeypatch, W, H, images, lights=True)
    assert_frames_identical(dense, sparse, ["zero", "lit", "dense"])
    assert sentinel_mask(sparse[0][0]["bloom"]).all()
    n_sent, n_written = check_cells(dense[0][1]["bloom"], sparse[0][1]["bloom"], "lit")
    assert n_sent > 0 and n_written > 0


def test_padded_offset_views(soc, monkeypatch):
    """mip3 (odd pitch and offset) and the bloom output (16-B padded rows, offset) as views of poisoned canvases: the
    padding is intact, and the frames equal the dense run on tight images."""
    W, H = 200, 72
    images = [zeros_u16(H, W), lit_u16(H, W, 124, 16)]
    dense = run(soc, monkeypatch, "0", W, H, images)
    sparse = run(soc, monkeypatch, "1", W, H, images, layout=("odd", "pad16"))
    assert_frames_identical(dense, sparse, ["zero", "lit"])
    assert sentinel_mask(sparse[0][0]["bloom"]).all()
    n_sent, n_written = check_cells(dense[0][1]["bloom"], sparse[0][1]["bloom"], "lit")
    assert n_sent > 0 and n_written > 0


@pytest.mark.parametrize("W,H", SMALL)
def test_in_kernel_bloom_path(soc, monkeypatch, W, H):
    """A high-priority sky lane: the last stage runs inside Composition (Up10Tile), behind the same cell proof. Zero, one
    lit texel and dense emissive identical to SOC_BLOOM_SPARSE=0."""
    images = [zeros_u16(H, W), lit_u16(H, W, 32, 16), lit_u16(H, W, W - 1, H - 1),
              random_rgba16(H, W, seed=45, hi=16.0).view(np.uint16)]
    dense, sparse = both(soc, monkeypatch, W, H, images, lane="high")
    assert_frames_identical(dense, sparse, ["zero", "lit", "lit corner", "dense"])
    # the in-kernel path was taken (the fourth pass recorded nothing) in the last frames of both runs
    assert sentinel_mask(sparse[0][-1]["bloom"]).all() and sentinel_mask(dense[0][-1]["bloom"]).all()
