"""The view helper of the padded-view tests (tests/views.py) on host tensors: the residues each layout promises, relative
to the canvas's own base, the view's contents, and that assert_padding_intact sees one flipped padding byte."""
import itertools

import pytest
import torch

import soc_real_time_renderer_amd as soc_pkg
import views

FORMATS = {
    "rgba16f": ((4,), torch.float16, 8),
    "d32f": ((), torch.float32, 4),
    "rgba8": ((4,), torch.uint8, 4),
    "r8": ((), torch.uint8, 1),
    "rgba32f": ((4,), torch.float32, 16),
}
WIDTHS = (64, 98, 97, 55, 48, 16, 136)      # even, odd and multiples of 16
H = 5


def _image(fmt, W, seed=0):
    tail, dtype, _ = FORMATS[fmt]
    gen = torch.Generator().manual_seed(seed + W)
    if dtype == torch.uint8:
        return torch.randint(0, 256, (H, W) + tail, dtype=torch.uint8, generator=gen)
    return torch.rand((H, W) + tail, generator=gen).to(dtype)


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("W", WIDTHS)
def test_layout_residues(fmt, W):
    _, _, bpp = FORMATS[fmt]
    t = _image(fmt, W)
    pitches = []
    for layout, index in [("pad16", 0), ("odd", 0)] + [("mixed", i) for i in range(6)]:
        for role in ("in", "out"):
            v, canvas = views.make_view(t, layout, index, role)
            im = soc_pkg.img(v)                       # the binding accepts every view the helper builds
            data = v.data_ptr() - canvas.data_ptr()
            pitch = v.stride(0) * v.element_size()
            assert im.pitch_bytes == pitch and im.width == W and im.height == H
            assert pitch > W * bpp
            assert data % bpp == 0 and pitch % bpp == 0
            # the guard: G rows above and below, at least one texel beside each row
            L = (data - views.G * pitch) // bpp
            assert canvas.shape[0] == H + 2 * views.G and L >= 1 and canvas.shape[1] - L - W >= 1
            kind = layout if layout != "mixed" else ("pad16" if index % 2 == 0 else "odd")
            if kind == "pad16":
                assert data % 16 == 0 and pitch % 16 == 0, (data, pitch)
            elif bpp == 8:
                assert data % 16 == 8 and pitch % 16 == 8, (data, pitch)
            elif bpp == 4:
                assert data % 8 == 4 and pitch % 8 == 4, (data, pitch)
            elif bpp == 1:
                assert data % 2 == 1 and pitch % 2 == 1, (data, pitch)
            else:
                assert L == 1 and (canvas.shape[1] - L - W) % 2 == 0
            assert views.bits_equal(v, t)
            views.assert_padding_intact(canvas, H, W, layout)
            if layout == "mixed" and role == "in":
                pitches.append(pitch)
    assert len(set(pitches)) == len(pitches), pitches      # no two images of a mixed call share a pitch


def test_tight_is_the_tensor_itself():
    t = _image("rgba16f", 64)
    v, canvas = views.make_view(t, "tight")
    assert v is t and canvas is None
    views.assert_padding_intact(canvas, H, 64, "tight")


@pytest.mark.parametrize("fmt,layout,role", list(itertools.product(FORMATS, views.LAYOUTS, ("in", "out"))))
def test_one_flipped_padding_byte_is_seen(fmt, layout, role):
    W = 33
    t = _image(fmt, W)
    _, canvas0 = views.make_view(t, layout, 1, role)
    nbytes = canvas0.numel() * canvas0.element_size()
    inside = ~views.padding_mask(canvas0, H, W, canvas0._view_geometry[2])
    tb = views.texel_bytes(t)
    # one byte each: the first and last of the canvas, the bytes just before and after the first and the last row
    L = canvas0._view_geometry[2]
    pitch = canvas0.stride(0) * canvas0.element_size()
    first = views.G * pitch + L * tb
    last = (views.G + H - 1) * pitch + L * tb
    for off in (0, nbytes - 1, first - 1, first + W * tb, last - 1, last + W * tb, last + pitch):
        v, canvas = views.make_view(t, layout, 1, role)
        raw = canvas.view(torch.uint8).reshape(-1)
        raw[off] ^= 0x10
        with pytest.raises(AssertionError, match="padding"):
            views.assert_padding_intact(canvas, H, W, layout, fmt)
    # a changed texel inside the view is not padding
    v, canvas = views.make_view(t, layout, 1, role)
    canvas.view(torch.uint8).reshape(-1)[first] ^= 0x10
    views.assert_padding_intact(canvas, H, W, layout)
    assert bool(inside.any())
