"""Padded, offset and misaligned image views for the view tests (test_views.py, test_gpu_views.py).

make_view(t, layout, index) copies an (H, W[, 4]) image into the interior of a poisoned canvas of
(H + 2G) x (L + W + R) texels and returns the interior view canvas[G:G+H, L:L+W] with the canvas. The guard rows and
columns (G = 2 rows above and below, L >= 1 and R >= 1 texels beside every row) hold the poison, so a store outside the
rows of the view shows in assert_padding_intact, and an access that strays by less than one pitch in either direction
stays inside the canvas's own allocation: no view's last row ends at the end of its allocation.

Layouts (bpp = bytes per texel; the residues are relative to the canvas's base, which torch allocates 256-byte
aligned on the device and which the CPU test subtracts):
  tight  the tensor itself.
  pad16  L * bpp % 16 == 0 and (L + W + R) * bpp % 16 == 0: data % 16 == 0 and pitch % 16 == 0, pitch != W * bpp.
  odd    L = 1 and an odd number of texels per canvas row: with G = 2, data = (2 * pitch + bpp) and so
         8-byte texels: pitch % 16 == 8, data % 16 == 8; 4-byte texels: pitch % 8 == 4, data % 8 == 4;
         R8: odd pitch, odd base; RGBA32F (16-byte texels cannot be misaligned by a texel offset): L = 1, R = 2.
  mixed  pad16 for an even `index`, odd for an odd one, R enlarged by `index` in steps that keep the layout's
         residues: no two images of a call share a pitch.
"""
import torch

G = 2
LAYOUTS = ("pad16", "odd", "mixed")

_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
# Output poisons: one fixed non-NaN bit pattern per dtype that no pass stores. float16 0x6A5B = 3254.0 and float32
# 0x4EADBEEF = 1.458e9 are finite values no pass computes from the tests' inputs (colours below 1e3, depths and tone
# mapped values in [0, 1]); uint8 0x5B: every byte of a written RGBA8 / R8 texel may equal it by chance, a row of them
# may not (the comparison is over the whole padding).
OUT_POISON = {torch.float16: 0x6A5B, torch.float32: 0x4EADBEEF, torch.uint8: 0x5B}
IN_POISON_U8 = 0xA5


def texel_bytes(t):
    return t.element_size() * (t.shape[2] if t.dim() == 3 else 1)


def _margins(W, bpp, layout, index):
    """(L, R) texels left and right of the view."""
    if layout == "mixed":
        layout = "pad16" if index % 2 == 0 else "odd"
        extra = index
    else:
        extra = 0
    if layout == "pad16":
        q = max(16 // bpp, 1)                 # texels per 16 bytes
        L = q
        R = q - (L + W) % q                   # in 1..q: the row is a whole number of 16-byte units
        return L, R + q * extra
    if layout == "odd":
        if bpp == 16:
            return 1, 2 + 2 * extra       # even; pad16's R is odd for 16-byte texels
        R = 1 if (1 + W + 1) % 2 == 1 else 2  # an odd number of texels per row
        return 1, R + 2 * extra
    raise ValueError(layout)


def _int_bits(t):
    """The tensor's elements as integers of the same width (NaN poison compares by bits)."""
    return t if not t.is_floating_point() else t.view(_INT_VIEW[t.element_size()])


def poison_value(dtype, role):
    """The poison as an integer bit pattern of one element."""
    if role == "in":
        return {torch.float16: 0x7E00, torch.float32: 0x7FC00000, torch.uint8: IN_POISON_U8}[dtype]
    return OUT_POISON[dtype]


def make_view(t, layout, index=0, role="in"):
    """(view, canvas): `t` copied into a poisoned canvas (see the module docstring). role "in": NaN (float) / 0xA5
    (uint8) poison; "out": OUT_POISON. `tight` returns (t, None)."""
    if layout == "tight":
        return t, None
    H, W = int(t.shape[0]), int(t.shape[1])
    L, R = _margins(W, texel_bytes(t), layout, index)
    shape = (H + 2 * G, L + W + R) + tuple(t.shape[2:])
    canvas = torch.empty(shape, dtype=t.dtype, device=t.device)
    _int_bits(canvas).fill_(_signed(poison_value(t.dtype, role), t.element_size()))
    view = canvas[G:G + H, L:L + W]
    view.copy_(t)
    canvas._view_geometry = (H, W, L, role)
    return view, canvas


def _signed(v, size):
    bits = 8 * size
    return v - (1 << bits) if size > 1 and v >= 1 << (bits - 1) else v


def padding_mask(canvas, H, W, L):
    m = torch.ones(canvas.shape[:2], dtype=torch.bool, device=canvas.device)
    m[G:G + H, L:L + W] = False
    return m


def assert_padding_intact(canvas, H, W, layout, what=""):
    """Every element of the canvas outside the view still holds the poison (compared as integers)."""
    if layout == "tight" or canvas is None:
        return
    h, w, L, role = canvas._view_geometry
    assert (h, w) == (H, W), (h, w, H, W)
    bits = _int_bits(canvas)
    want = _signed(poison_value(canvas.dtype, role), canvas.element_size())
    bad = (bits != want)
    if bad.dim() == 3:
        bad = bad.any(dim=2)
    bad &= padding_mask(canvas, H, W, L)
    n = int(bad.sum())
    if n:
        ys, xs = torch.nonzero(bad, as_tuple=True)
        first = [(int(y) - G, int(x) - L) for y, x in zip(ys[:6].tolist(), xs[:6].tolist())]
        raise AssertionError(f"{what}: {n} padding texels of the {tuple(canvas.shape)} canvas around the {H}x{W} view "
                             f"(layout {layout}) were overwritten; first at (row, column) relative to the view: {first}")


def bits_equal(a, b):
    """torch.equal on integer views (NaNs and signed zeros compare by bits)."""
    return a.shape == b.shape and torch.equal(_int_bits(a.contiguous()), _int_bits(b.contiguous()))
