"""soc_depth_of_field_chain_bytes / soc_depth_of_field_mips / soc_depth_of_field / soc_renderer_add_depth_of_field:
argument checks and the passes' place in the render graph (CPU only: validation happens before any HIP call, the graph
is built and inspected, nothing is launched)."""
import ctypes as C

import numpy as np
import pytest
import torch

W, H = 128, 64


def _chain_np(soc, w=W, h=H, pitch=None):
    """(flat uint8 allocation, float16 level-0 view) on the host."""
    pitch = pitch or 8 * w
    buf = np.zeros(int(soc.lib().soc_depth_of_field_chain_bytes(w, h, pitch)), np.uint8)
    lv0 = np.lib.stride_tricks.as_strided(buf[:pitch * h].view(np.float16), (h, w, 4), (pitch, 8, 2))
    return buf, lv0


def _images(soc, w=W, h=H):
    buf, lv0 = _chain_np(soc, w, h)
    return {"depth": np.ones((h, w), np.float32), "color": np.zeros((h, w, 4), np.float16), "chain": lv0,
            "target": np.zeros((h, w, 4), np.float16), "_buf": buf}


def _mips(soc, im, **replace):
    a = {k: soc.img(v) for k, v in im.items() if not k.startswith("_")}
    a.update(replace)
    rc = soc.lib().soc_depth_of_field_mips(a["color"], a["chain"], None)
    return rc, soc.lib().soc_last_error_string().decode()


def _dof(soc, g, im, **replace):
    a = {k: soc.img(v) for k, v in im.items() if not k.startswith("_")}
    a.update(replace)
    rc = soc.lib().soc_depth_of_field(C.byref(g) if g is not None else None, a["depth"], a["chain"], a["target"], None)
    return rc, soc.lib().soc_last_error_string().decode()


def test_chain_bytes(soc):
    f = soc.lib().soc_depth_of_field_chain_bytes
    # 97x55: 7 levels, 97x55, 48x27, 24x13, 12x6, 6x3, 3x1, 1x1
    tail = 48 * 27 + 24 * 13 + 12 * 6 + 6 * 3 + 3 * 1 + 1
    assert f(97, 55, 97 * 8) == 8 * (97 * 55 + tail)
    assert f(97, 55, 104 * 8) == 8 * (104 * 55 + tail)          # a padded level 0; the rest is tight
    assert f(1, 1, 8) == 8 and f(1, 1, 24) == 24
    assert f(3840, 2160, 3840 * 8) == 8 * sum(max(1, 3840 >> k) * max(1, 2160 >> k) for k in range(12))
    for bad in ((0, 55, 800), (97, -1, 800), (97, 55, 97 * 8 - 8), (97, 55, 97 * 8 + 4), (8193, 1, 8193 * 8), (1, 8193, 8)):
        assert f(*bad) == 0, bad
    ch = soc.depth_of_field_chain(97, 55, device="cpu")
    assert ch.buf.numel() == f(97, 55, 97 * 8)
    assert [tuple(lv.shape) for lv in ch.levels()] == [(55, 97, 4), (27, 48, 4), (13, 24, 4), (6, 12, 4), (3, 6, 4), (1, 3, 4),
                                                      (1, 1, 4)]
    assert ch.levels()[1].data_ptr() == ch.buf.data_ptr() + 8 * 97 * 55


def test_argument_errors(soc):
    E_ARG, E_SHAPE = soc._abi.SOC_E_INVALID_ARG, soc._abi.SOC_E_SHAPE
    g = soc.globals_defaults(W, H)
    im = _images(soc)
    none = soc.SocImg(None, 0, 0, 0, 0)
    rc, msg = _dof(soc, None, im)
    assert rc == E_ARG and "soc_depth_of_field" in msg
    for name in ("depth", "chain", "target"):
        rc, msg = _dof(soc, g, im, **{name: none})
        assert rc == E_ARG and "soc_depth_of_field:" in msg and name in msg, (name, msg)
    for name in ("color", "chain"):
        rc, msg = _mips(soc, im, **{name: none})
        assert rc == E_ARG and "soc_depth_of_field_mips" in msg and name in msg, (name, msg)
    # wrong formats
    rc, msg = _dof(soc, g, im, depth=soc.img(im["color"]))
    assert rc == E_ARG and "depth" in msg and "format" in msg
    for name in ("chain", "target"):
        rc, msg = _dof(soc, g, im, **{name: soc.img(im["depth"])})
        assert rc == E_ARG and name in msg and "format" in msg
    rc, msg = _dof(soc, g, im, target=soc.img(np.zeros((H, W, 4), np.uint8)))
    assert rc == E_ARG and "target" in msg
    for name in ("color", "chain"):
        rc, msg = _mips(soc, im, **{name: soc.img(im["depth"])})
        assert rc == E_ARG and "soc_depth_of_field_mips" in msg and name in msg and "format" in msg
    # mismatched extents
    small = _images(soc, W - 1, H)
    for name in ("depth", "chain"):
        rc, msg = _dof(soc, g, im, **{name: soc.img(small[name])})
        assert rc == E_SHAPE and "soc_depth_of_field:" in msg and name in msg, (name, msg)
    rc, msg = _dof(soc, g, im, target=soc.img(small["target"]))
    assert rc == E_SHAPE and "soc_depth_of_field:" in msg
    rc, msg = _mips(soc, im, color=soc.img(small["color"]))
    assert rc == E_SHAPE and "soc_depth_of_field_mips" in msg
    # a base or a pitch that is no multiple of the texel size (no tensor view has one: built by hand)
    for call, names in ((_dof, ("depth", "chain", "target")), (_mips, ("color", "chain"))):
        for name in names:
            ok = soc.img(im[name])
            b = im[name].strides[1]
            for data, pitch in ((ok.data + b // 2, ok.pitch_bytes), (ok.data, ok.pitch_bytes + b // 2)):
                bad = soc.SocImg(data, W, H - 1, pitch, ok.format)
                rc, msg = call(soc, g, im, **{name: bad}) if call is _dof else call(soc, im, **{name: bad})
                assert rc == E_ARG and "soc_depth_of_field" in msg and "aligned" in msg and name in msg, (name, msg)
    # an extent above 8192 (one row: validation reads no texel; the chain view is hand-built, no allocation that long)
    wide = {"depth": np.ones((1, 8193), np.float32), "color": np.zeros((1, 8193, 4), np.float16),
            "chain": np.zeros((1, 8193, 4), np.float16), "target": np.zeros((1, 8193, 4), np.float16)}
    rc, msg = _dof(soc, g, wide)
    assert rc == E_ARG and "8192" in msg and "soc_depth_of_field:" in msg
    rc, msg = _mips(soc, wide)
    assert rc == E_ARG and "8192" in msg and "soc_depth_of_field_mips" in msg
    with pytest.raises(soc.SocError, match="soc_depth_of_field"):
        soc.depth_of_field(g, None, None, None, stream=0)
    with pytest.raises(soc.SocError, match="soc_depth_of_field_mips"):
        soc.depth_of_field_mips(None, None, stream=0)


def test_target_may_not_alias_the_chain(soc):
    E_ARG = soc._abi.SOC_E_INVALID_ARG
    g = soc.globals_defaults(W, H)
    im = _images(soc)
    buf = im["_buf"]
    # level 0 itself, and a W x 1 view over the last bytes of the allocation (the 1x1 level's texel is its last)
    rc, msg = _dof(soc, g, im, target=soc.img(im["chain"]))
    assert rc == E_ARG and "alias" in msg and "soc_depth_of_field:" in msg
    last = soc.SocImg(buf.ctypes.data + buf.size - 8, W, H, 8 * W, soc.FMT_RGBA16F)
    rc, msg = _dof(soc, g, im, target=last)
    assert rc == E_ARG and "alias" in msg
    before = soc.SocImg(buf.ctypes.data - 8 * W * (H - 1) - 8, W, H, 8 * W, soc.FMT_RGBA16F)   # its last texel is the chain's first
    rc, msg = _dof(soc, g, im, target=before)
    assert rc == E_ARG and "alias" in msg
    rc, msg = _mips(soc, im, color=soc.img(im["chain"]))
    assert rc == E_ARG and "alias" in msg and "soc_depth_of_field_mips" in msg


def _renderer(soc, **kw):
    fr = soc.alloc_frame(W, H, device="cpu", noise_table=False)
    return soc.Renderer(fr, **kw)


UNFUSED = dict(fused_histogram=False)


def _deps(r):
    names = r.pass_names()
    return {names[i]: {names[j] for j in r.pass_dependencies(i)} for i in range(len(names))}


def _raster_scene(soc, r):
    sc = soc._abi.RasterScene()
    for f in ("positions", "normals", "uvs", "indices"):
        setattr(sc.mesh, f, 1)
    sc.mesh.vertex_count, sc.mesh.triangle_count = 3, 1
    sc.materials, sc.material_count, sc.shadow, sc.visibility, sc.workspace = 1, 1, 1, 1, 1
    assert soc.lib().soc_renderer_set_raster_scene(r.handle, C.byref(sc)) == 0


@pytest.mark.parametrize("kw", [UNFUSED, dict(fused_bloom=False, fused_tonemap=False, fused_histogram=False)])
def test_passes_sit_where_the_reference_has_them(soc, kw):
    """renderer.cpp:1119-1153: after Composition, directly before GenerateLuminanceHistogram, group "Depth Of Field"."""
    plain = _renderer(soc, **kw).pass_names()
    r = _renderer(soc, **kw)
    r.add_depth_of_field(soc.depth_of_field_chain(W, H, device="cpu"))

    def check():
        names = r.pass_names()
        i = names.index("MipMapping")
        assert names[i + 1] == "DepthOfField" and names[i + 2] == "GenerateLuminanceHistogram"
        assert r.pass_groups()[i] == r.pass_groups()[i + 1] == "Depth Of Field"
        assert r.pass_uses(i) == ({"COLOR"}, {"USER0"})
        assert r.pass_uses(i + 1) == ({"USER0", "DEPTH"}, {"COLOR"})
        assert r.pass_lane(i) == 0 and r.pass_lane(i + 1) == 0
        deps = _deps(r)
        assert "Composition" in deps["MipMapping"]
        assert "MipMapping" in deps["DepthOfField"]
        assert "DepthOfField" in deps["GenerateLuminanceHistogram"]
        taa = next(n for n in names if n.startswith("TemporalAntiAliasing"))
        assert "DepthOfField" in deps[taa]
        return names, i
    names, i = check()
    assert names[:i] + names[i + 2:] == plain
    assert names[i - 1] == "Composition"
    _raster_scene(soc, r)                      # the pair survives the rebuild
    names, i = check()
    assert "GBufferGeneration" in names


def test_resource_and_anchor(soc):
    r = _renderer(soc, **UNFUSED)
    r.add_depth_of_field(soc.depth_of_field_chain(W, H, device="cpu"), chain_resource=soc._abi.RES_USER0 + 31, before="Composition")
    names = r.pass_names()
    i = names.index("MipMapping")
    assert names[i + 1:i + 3] == ["DepthOfField", "Composition"]
    assert r.pass_uses(i) == ({"COLOR"}, {"USER31"}) and r.pass_uses(i + 1) == ({"USER31", "DEPTH"}, {"COLOR"})


def test_add_errors_leave_the_graph_unchanged(soc):
    chain = soc.depth_of_field_chain(W, H, device="cpu")
    fused = _renderer(soc)
    n0, d0 = fused.pass_names(), _deps(fused)
    with pytest.raises(soc.SocError, match="SOC_RENDERER_UNFUSED_HISTOGRAM.*histogram"):
        fused.add_depth_of_field(chain)
    assert fused.pass_names() == n0 and _deps(fused) == d0
    r = _renderer(soc, **UNFUSED)
    n0, d0 = r.pass_names(), _deps(r)
    with pytest.raises(soc.SocError, match="bad resource"):
        r.add_depth_of_field(chain, chain_resource="DEPTH")
    with pytest.raises(soc.SocError, match="bad resource"):
        r.add_depth_of_field(chain, chain_resource=64)
    with pytest.raises(soc.SocError, match="no pass named"):
        r.add_depth_of_field(chain, before="NoSuchPass")
    with pytest.raises(soc.SocError, match="another phase"):
        r.add_depth_of_field(chain, before="ResolveLuminanceHistogram")
    with pytest.raises(soc.SocError, match="soc_renderer_add_depth_of_field"):
        r.add_depth_of_field(None)
    with pytest.raises(soc.SocError, match="soc_renderer_add_depth_of_field"):
        r.add_depth_of_field(soc.depth_of_field_chain(W - 2, H, device="cpu"))
    with pytest.raises(soc.SocError, match="soc_renderer_add_depth_of_field.*format"):
        r.add_depth_of_field(torch.zeros(H, W, dtype=torch.float32))
    with pytest.raises(soc.SocError, match="alias"):
        r.add_depth_of_field(r.frame["color"])
    assert soc.lib().soc_renderer_add_depth_of_field(None, soc.img(chain.level0), 32, None) == soc._abi.SOC_E_INVALID_ARG
    assert r.pass_names() == n0 and _deps(r) == d0
    # a caller pass that already holds the second name: the first registration is rolled back
    r.add_pass("DepthOfField", lambda *a: 0)
    n1, d1 = r.pass_names(), _deps(r)
    with pytest.raises(soc.SocError, match="duplicate"):
        r.add_depth_of_field(chain)
    assert r.pass_names() == n1 and _deps(r) == d1 and "MipMapping" not in n1
    # a second add is a duplicate name, and leaves the graph with the one pair
    r2 = _renderer(soc, **UNFUSED)
    r2.add_depth_of_field(chain)
    n2, d2 = r2.pass_names(), _deps(r2)
    with pytest.raises(soc.SocError, match="duplicate"):
        r2.add_depth_of_field(chain)
    assert r2.pass_names() == n2 and _deps(r2) == d2
    assert n2.count("MipMapping") == 1 and n2.count("DepthOfField") == 1


def test_default_graph_has_no_depth_of_field(soc):
    """Opt-in: a renderer that never adds the passes runs the graph test_render_graph.py pins."""
    for kw in ({}, dict(fused_bloom=False, fused_tonemap=False, fused_histogram=False)):
        r = _renderer(soc, **kw)
        assert "MipMapping" not in r.pass_names() and "DepthOfField" not in r.pass_names()
        assert "Depth Of Field" not in r.pass_groups()
    assert soc.lib().soc_abi_version() == 1
