"""soc_screen_space_reflection / soc_renderer_add_screen_space_reflection: argument checks and the pass's place in the
render graph (CPU only: validation happens before any HIP call, the graph is built and inspected, nothing is launched)."""
import ctypes as C

import numpy as np
import pytest
import torch

W, H = 128, 64


def _images(w=W, h=H):
    f16 = lambda: np.zeros((h, w, 4), np.float16)   # noqa: E731
    return {"depth": np.ones((h, w), np.float32), "normal": f16(), "albedo": f16(), "mr": f16(), "target": f16(),
            "steps": np.zeros((h, w), np.uint8)}


def _call(soc, g, im, **replace):
    a = {k: soc.img(v) for k, v in im.items()}
    a.update(replace)
    rc = soc.lib().soc_screen_space_reflection(C.byref(g) if g is not None else None, a["depth"], a["normal"], a["albedo"],
                                               a["mr"], a["target"], a["steps"], None)
    return rc, soc.lib().soc_last_error_string().decode()


def test_argument_errors(soc):
    E_ARG, E_SHAPE = soc._abi.SOC_E_INVALID_ARG, soc._abi.SOC_E_SHAPE
    g = soc.globals_defaults(W, H)
    im = _images()
    none = soc.SocImg(None, 0, 0, 0, 0)
    rc, msg = _call(soc, None, im)
    assert rc == E_ARG and "soc_screen_space_reflection" in msg
    for name in ("depth", "normal", "albedo", "mr", "target"):
        rc, msg = _call(soc, g, im, **{name: none})
        assert rc == E_ARG and "soc_screen_space_reflection" in msg, name
    # wrong formats: a D32 image where RGBA16F is expected and the other way round, a float steps image
    rc, msg = _call(soc, g, im, mr=soc.img(im["depth"]))
    assert rc == E_ARG and "metallic_roughness" in msg and "format" in msg
    rc, msg = _call(soc, g, im, depth=soc.img(im["normal"]))
    assert rc == E_ARG and "depth" in msg
    rc, msg = _call(soc, g, im, target=soc.img(np.zeros((H, W, 4), np.uint8)))
    assert rc == E_ARG and "target" in msg
    rc, msg = _call(soc, g, im, steps=soc.img(im["depth"]))
    assert rc == E_ARG and "steps" in msg
    # mismatched extents
    small = _images(W - 1, H)
    for name in ("depth", "normal", "albedo", "mr", "steps"):
        rc, msg = _call(soc, g, im, **{name: soc.img(small[name])})
        assert rc == E_SHAPE and "soc_screen_space_reflection" in msg, name
    # a base or a pitch that is no multiple of the texel size (no tensor view has one: built by hand)
    for name in ("depth", "normal", "albedo", "mr", "target"):
        ok = soc.img(im[name])
        b = im[name].strides[1]
        for data, pitch in ((ok.data + b // 2, ok.pitch_bytes), (ok.data, ok.pitch_bytes + b // 2)):
            rc, msg = _call(soc, g, im, **{name: soc.SocImg(data, W, H - 1, pitch, ok.format)})
            assert rc == E_ARG and "soc_screen_space_reflection" in msg and "aligned" in msg, (name, msg)
            assert {"mr": "metallic_roughness"}.get(name, name) in msg
    # an extent above 8192 (one row: validation reads no texel)
    wide = _images(8193, 1)
    rc, msg = _call(soc, g, wide)
    assert rc == E_ARG and "8192" in msg and "soc_screen_space_reflection" in msg
    with pytest.raises(soc.SocError, match="soc_screen_space_reflection"):
        soc.screen_space_reflection(g, None, None, None, None, None, stream=0)


def _renderer(soc, **kw):
    fr = soc.alloc_frame(W, H, device="cpu", noise_table=False)
    return soc.Renderer(fr, **kw)


def _ssr_images():
    return (torch.zeros(H, W, 4, dtype=torch.float16), torch.zeros(H, W, 4, dtype=torch.float16),
            torch.zeros(H, W, dtype=torch.uint8))


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


@pytest.mark.parametrize("kw", [{}, dict(fused_bloom=False, fused_tonemap=False, fused_histogram=False)])
@pytest.mark.parametrize("async_compute", [False, True])
def test_pass_sits_where_the_reference_registers_it(soc, kw, async_compute):
    """renderer.cpp:1081-1092: after SSAOBlur, before CloudRendering, in the "Screen Space Reflections" metric group."""
    plain = _renderer(soc, **kw).pass_names()
    r = _renderer(soc, **kw)
    mr, target, steps = _ssr_images()
    r.add_screen_space_reflection(mr, target, steps, async_compute=async_compute)
    names = r.pass_names()
    i = names.index("ScreenSpaceReflection")
    assert names[i - 1] == "SSAOBlur" and names[i + 1] == "CloudRendering"
    assert names[:i] + names[i + 1:] == plain
    assert r.pass_groups()[i] == "Screen Space Reflections"
    assert r.pass_uses(i) == ({"ALBEDO", "NORMAL", "DEPTH", "USER0"}, {"USER1"})
    assert r.pass_lane(i) == (1 if async_compute else 0)
    # the G-buffer is an input of the frame: nothing in the frame precedes the pass, and nothing waits for it
    assert r.pass_dependencies(i) == []
    assert all("ScreenSpaceReflection" not in d for d in _deps(r).values())
    # with a raster head the G-buffer pass writes what it reads; it survives the rebuild
    _raster_scene(soc, r)
    names = r.pass_names()
    i = names.index("ScreenSpaceReflection")
    assert names[i - 1] == "SSAOBlur" and names[i + 1] == "CloudRendering"
    assert "GBufferGeneration" in {names[j] for j in r.pass_dependencies(i)}
    assert r.pass_lane(i) == (1 if async_compute else 0)


def test_resources_and_anchor(soc):
    r = _renderer(soc)
    mr, target, _ = _ssr_images()
    r.add_screen_space_reflection(mr, target, mr_resource="USER5", target_resource=soc._abi.RES_USER0 + 31,
                                  before="SSAOGeneration")
    names = r.pass_names()
    i = names.index("ScreenSpaceReflection")
    assert names[i + 1] == "SSAOGeneration"
    assert r.pass_uses(i) == ({"ALBEDO", "NORMAL", "DEPTH", "USER5"}, {"USER31"})
    # a caller pass that reads the ssr image is ordered after the pass
    r.add_pass("UseSSR", lambda *a: 0, reads=[soc._abi.RES_USER0 + 31], before="Composition+GenerateLuminanceHistogram")
    assert _deps(r)["UseSSR"] == {"ScreenSpaceReflection"}


def test_add_errors_leave_the_graph_unchanged(soc):
    r = _renderer(soc)
    n0 = r.pass_names()
    mr, target, steps = _ssr_images()
    with pytest.raises(soc.SocError, match="bad resource"):
        r.add_screen_space_reflection(mr, target, mr_resource="DEPTH")
    with pytest.raises(soc.SocError, match="bad resource"):
        r.add_screen_space_reflection(mr, target, target_resource=64)
    with pytest.raises(soc.SocError, match="no pass named"):
        r.add_screen_space_reflection(mr, target, before="NoSuchPass")
    with pytest.raises(soc.SocError, match="another phase"):
        r.add_screen_space_reflection(mr, target, before="ResolveLuminanceHistogram")
    with pytest.raises(soc.SocError, match="soc_renderer_add_screen_space_reflection"):
        r.add_screen_space_reflection(None, target)
    with pytest.raises(soc.SocError, match="soc_renderer_add_screen_space_reflection"):
        r.add_screen_space_reflection(mr, torch.zeros(H, W - 2, 4, dtype=torch.float16))
    lib = soc.lib()
    assert lib.soc_renderer_add_screen_space_reflection(None, soc.img(mr), soc.img(target), soc.img(None), 32, 33, 0,
                                                        None) == soc._abi.SOC_E_INVALID_ARG
    assert lib.soc_renderer_add_screen_space_reflection(r.handle, soc.img(mr), soc.img(target), soc.img(None), 32, 33, 2,
                                                        None) == soc._abi.SOC_E_INVALID_ARG
    assert r.pass_names() == n0
    # a second add is a duplicate name, and leaves the graph with the one pass
    r.add_screen_space_reflection(mr, target, steps)
    n1 = r.pass_names()
    d1 = _deps(r)
    assert n1.count("ScreenSpaceReflection") == 1
    with pytest.raises(soc.SocError, match="duplicate"):
        r.add_screen_space_reflection(mr, target, steps)
    assert r.pass_names() == n1 and _deps(r) == d1


def test_default_graph_has_no_ssr(soc):
    """Opt-in: a renderer that never adds the pass runs the graph test_render_graph.py pins."""
    for kw in ({}, dict(fused_bloom=False, fused_tonemap=False, fused_histogram=False)):
        r = _renderer(soc, **kw)
        assert "ScreenSpaceReflection" not in r.pass_names()
        assert "Screen Space Reflections" not in r.pass_groups()
    assert soc.lib().soc_abi_version() == 1
