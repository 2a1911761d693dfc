"""The terrain layer through the C ABI without a GPU: the struct layout, every host-side refusal of soc_draw_terrain,
soc_sun_shadow_draw_terrain and soc_renderer_set_terrain (made before any HIP call: the pointers here are not device
memory, reaching a launch would not return an error code) and the render graph's two passes (built and inspected, nothing
is launched)."""
import ctypes as C

import numpy as np
import pytest

from soc_real_time_renderer_amd import _abi, raster
from test_draws_abi import _renderer, _scene

E_ARG, E_SHAPE = _abi.SOC_E_INVALID_ARG, _abi.SOC_E_SHAPE
LAYER_USES = {"VISIBILITY", "DEPTH", "ALBEDO", "NORMAL", "VELOCITY"}


def test_struct_layout_matches_the_ctypes_mirror(soc):
    lib, st = soc.lib(), _abi.TerrainLayer
    assert lib.soc_abi_sizeof(b"soc_terrain_layer") == C.sizeof(st)
    for fname, _ in st._fields_:
        assert lib.soc_abi_offsetof(b"soc_terrain_layer", fname.encode()) == getattr(st, fname).offset, fname
    assert C.sizeof(st) == 2 * C.sizeof(_abi.Mesh) + 40
    assert lib.soc_abi_version() == 1


def _mesh(**replace):
    m = _abi.Mesh()
    for f in ("positions", "normals", "uvs", "indices"):
        setattr(m, f, 256)
    m.vertex_count, m.triangle_count = 3, 1
    for k, v in replace.items():
        setattr(m, k, v)
    return m


def _rc(soc, fn, *args):
    rc = fn(*args)
    return rc, soc.lib().soc_last_error_string().decode()


def test_direct_calls_refuse_on_the_host(soc):
    lib = soc.lib()
    g = soc.globals_defaults(64, 36)
    vis = np.zeros((36, 64), np.uint64)
    f16 = lambda h=36, w=64: soc.img(np.zeros((h, w, 4), np.float16))   # noqa: E731
    depth = soc.img(np.ones((36, 64), np.float32))
    ok = dict(g=C.byref(g), mesh=C.byref(_mesh()), mats=256, count=1, vis=vis.ctypes.data, depth=depth, albedo=f16(),
              normal=f16(), velocity=f16(), ws=4096)

    def draw(**kw):
        a = dict(ok, **kw)
        return _rc(soc, lib.soc_draw_terrain, a["g"], a["mesh"], a["mats"], a["count"], a["vis"], a["depth"], a["albedo"],
                   a["normal"], a["velocity"], a["ws"], None)
    for kw in (dict(g=None), dict(mesh=None), dict(mats=None), dict(vis=None), dict(ws=None), dict(count=0), dict(count=-1),
               dict(mesh=C.byref(_mesh(positions=None))), dict(mesh=C.byref(_mesh(indices=None))),
               dict(mesh=C.byref(_mesh(normals=None))), dict(mesh=C.byref(_mesh(uvs=None))),
               dict(mesh=C.byref(_mesh(vertex_count=-1))), dict(mesh=C.byref(_mesh(triangle_count=-1)))):
        rc, msg = draw(**kw)
        assert rc == E_ARG and "soc_draw_terrain" in msg, (kw, rc, msg)
    # wrong formats: every image in turn (a D32 image where RGBA16F is wanted and the other way round)
    for name in ("albedo", "normal", "velocity"):
        rc, msg = draw(**{name: depth})
        assert rc == E_ARG and name in msg and "soc_draw_terrain" in msg, msg
    rc, msg = draw(depth=f16())
    assert rc == E_ARG and "depth" in msg
    rc, msg = draw(albedo=soc.SocImg(None, 0, 0, 0, 0))
    assert rc == E_ARG and "albedo" in msg
    # differing extents
    for name in ("albedo", "normal", "velocity"):
        rc, msg = draw(**{name: f16(36, 60)})
        assert rc == E_SHAPE and "extent" in msg, (name, msg)

    vp = (C.c_float * 16)()

    def shadow(mesh=ok["mesh"], m=vp, clear=0, d=depth, ws=4096):
        return _rc(soc, lib.soc_sun_shadow_draw_terrain, mesh, m, clear, d, ws, None)
    for kw in (dict(mesh=None), dict(m=None), dict(ws=None), dict(mesh=C.byref(_mesh(positions=None))),
               dict(mesh=C.byref(_mesh(indices=None))), dict(d=f16()), dict(d=soc.SocImg(None, 0, 0, 0, 0))):
        for clear in (0, 1):
            rc, msg = shadow(clear=clear, **kw)
            assert rc == E_ARG and "soc_sun_shadow_draw_terrain" in msg, (kw, msg)
    # a shadow mesh needs no normals or uvs: it gets past the mesh check to the next refusal
    rc, msg = shadow(mesh=C.byref(_mesh(normals=None, uvs=None)), ws=None)
    assert rc == E_ARG and "workspace" in msg


def _layer(**replace):
    t = _abi.TerrainLayer()
    t.mesh = _mesh()
    t.materials, t.material_count, t.shadow = 256, 1, 1
    t.visibility, t.workspace, t.shadow_workspace = 256, 4096, 8192
    for k, v in replace.items():
        setattr(t, k, v)
    return t


def _mesh_head(shadow=1):
    rs = _abi.RasterScene()
    rs.mesh = _mesh()
    rs.materials, rs.material_count, rs.shadow, rs.visibility, rs.workspace = 1, 1, shadow, 1, 1
    return rs


def _set_head(soc, r, kind, shadow):
    lib = soc.lib()
    if kind == "mesh":
        return lib.soc_renderer_set_raster_scene(r.handle, C.byref(_mesh_head(shadow)))
    sc = _scene([raster.draw(0, 10, 0, 30, transform=1, material=1)])
    return lib.soc_renderer_set_draw_scene(r.handle, C.byref(sc), 256, 2, shadow, 256)


def _describe(r):
    n = len(r.pass_names())
    return [(name, group, r.pass_uses(i), r.pass_dependencies(i), r.pass_carry_dependencies(i), r.pass_lane(i))
            for i, (name, group) in enumerate(zip(r.pass_names(), r.pass_groups()))][:n]


def test_set_terrain_refusals(soc):
    lib = soc.lib()
    rc, msg = _rc(soc, lib.soc_renderer_set_terrain, None, C.byref(_layer()))
    assert rc == E_ARG and "soc_renderer_set_terrain" in msg
    r = _renderer(soc)
    names0 = r.pass_names()
    rc, msg = _rc(soc, lib.soc_renderer_set_terrain, r.handle, C.byref(_layer()))
    assert rc == E_ARG and "head" in msg                                      # no raster head
    assert lib.soc_renderer_set_terrain(r.handle, None) == 0                  # removing what is not there is fine
    assert r.pass_names() == names0
    assert _set_head(soc, r, "mesh", 1) == 0
    head = _describe(r)
    bad_mesh = [_mesh(**{f: None}) for f in ("positions", "normals", "uvs", "indices")] + [_mesh(vertex_count=-1)]
    for kw in ([dict(materials=None), dict(material_count=0), dict(visibility=None), dict(workspace=None),
                dict(shadow_workspace=None), dict(shadow_mesh=_mesh(indices=None))] + [dict(mesh=m) for m in bad_mesh]):
        rc, msg = _rc(soc, lib.soc_renderer_set_terrain, r.handle, C.byref(_layer(**kw)))
        assert rc == E_ARG and "soc_renderer_set_terrain" in msg, (kw, msg)
        assert _describe(r) == head                                           # errors leave the graph as it was
    # without the shadow pass neither a shadow workspace nor a shadow mesh is looked at
    assert lib.soc_renderer_set_terrain(r.handle, C.byref(_layer(shadow=0, shadow_workspace=None))) == 0
    assert "DrawTerrain" in r.pass_names() and "SunShadowDrawTerrain" not in r.pass_names()
    with pytest.raises(soc.SocError, match="soc_renderer_set_terrain"):
        r.set_terrain(raster.MeshBuffers(*(np.zeros((3, k), np.float32) for k in (3, 3, 2)), np.zeros((1, 3), np.uint32)),
                      None, 1, None, None)


@pytest.mark.parametrize("kind", ["mesh", "draws"])
@pytest.mark.parametrize("head_shadow", [1, 0])
def test_the_two_passes_in_the_graph(soc, kind, head_shadow):
    lib = soc.lib()
    plain = _renderer(soc)
    assert _set_head(soc, plain, kind, head_shadow) == 0
    head = _describe(plain)
    head_names = [p[0] for p in head]
    r = _renderer(soc)
    assert _set_head(soc, r, kind, head_shadow) == 0
    assert _describe(r) == head
    assert lib.soc_renderer_set_terrain(r.handle, C.byref(_layer())) == 0
    names = r.pass_names()
    # exactly the head's passes in their order, plus the two new ones at their places
    assert [n for n in names if n not in ("DrawTerrain", "SunShadowDrawTerrain")] == head_names
    at = {n: i for i, n in enumerate(names)}
    assert at["DrawTerrain"] == at["GBufferGeneration"] + 1
    assert at["SunShadowDrawTerrain"] == at["SunShadowDraw" if head_shadow else "DepthPrepass"] + 1
    assert r.pass_groups()[at["DrawTerrain"]] == "Rendering G-Buffer"
    assert r.pass_groups()[at["SunShadowDrawTerrain"]] == "Shadows"
    reads, writes = r.pass_uses(at["DrawTerrain"])
    assert set(reads) == LAYER_USES and set(writes) == LAYER_USES
    reads, writes = r.pass_uses(at["SunShadowDrawTerrain"])
    assert set(reads) == {"SUN_SHADOW"} and set(writes) == {"SUN_SHADOW"}
    # lanes: DrawTerrain on the caller's stream; the terrain shadow where the head's shadow draw runs, else the caller's
    assert r.pass_lane(at["DrawTerrain"]) == 0
    want_lane = r.pass_lane(at["SunShadowDraw"]) if head_shadow else 0
    assert r.pass_lane(at["SunShadowDrawTerrain"]) == want_lane
    if kind == "draws" and head_shadow:
        assert want_lane == 1                                                # the draw workspace holds the sun view's buffers
    # derived dependencies: DrawTerrain follows GBufferGeneration (every image it loads) and nothing else of the head
    deps = r.pass_dependencies(at["DrawTerrain"])
    assert at["GBufferGeneration"] in deps and all(d < at["DrawTerrain"] for d in deps)
    sdeps = r.pass_dependencies(at["SunShadowDrawTerrain"])
    assert sdeps == ([at["SunShadowDraw"]] if head_shadow else [])
    # every later reader of an image the layer writes now follows the layer, not GBufferGeneration directly
    for i, n in enumerate(names):
        rd, wr = r.pass_uses(i)
        if i > at["DrawTerrain"] and (set(rd) | set(wr)) & (LAYER_USES - {"VISIBILITY"}):
            assert any(d >= at["DrawTerrain"] for d in r.pass_dependencies(i)), n
        if i > at["SunShadowDrawTerrain"] and "SUN_SHADOW" in rd:
            assert at["SunShadowDrawTerrain"] in r.pass_dependencies(i), n   # the last writer of the shadow image
    # ring edges: the next frame's head shadow draw (or, without one, the clearing terrain draw) rewrites the shadow
    # image the previous frame's readers may still hold: the first SUN_SHADOW writer carries them
    first_writer = at["SunShadowDraw"] if head_shadow else at["SunShadowDrawTerrain"]
    readers = [i for i in range(len(names)) if "SUN_SHADOW" in r.pass_uses(i)[0] and i not in
               (at["SunShadowDrawTerrain"],)]
    assert set(readers) <= set(r.pass_carry_dependencies(first_writer)) | {first_writer}
    with_layer = _describe(r)

    # the layer survives replacing the head by another head (either kind)
    other = "draws" if kind == "mesh" else "mesh"
    assert _set_head(soc, r, other, head_shadow) == 0
    assert "DrawTerrain" in r.pass_names() and "SunShadowDrawTerrain" in r.pass_names()
    assert r.pass_names().index("DrawTerrain") == r.pass_names().index("GBufferGeneration") + 1
    assert _set_head(soc, r, kind, head_shadow) == 0
    assert _describe(r) == with_layer
    # a head without / with the shadow draw moves the terrain shadow pass and flips its clear
    assert _set_head(soc, r, kind, 1 - head_shadow) == 0
    names2 = r.pass_names()
    assert names2.index("SunShadowDrawTerrain") == names2.index("SunShadowDraw" if not head_shadow else "DepthPrepass") + 1
    assert _set_head(soc, r, kind, head_shadow) == 0
    # set_terrain(NULL) removes it: the head's graph again
    assert lib.soc_renderer_set_terrain(r.handle, None) == 0
    assert _describe(r) == head
    # it is removed with the head, and does not come back with the next one
    assert lib.soc_renderer_set_terrain(r.handle, C.byref(_layer())) == 0
    assert lib.soc_renderer_set_raster_scene(r.handle, None) == 0
    assert r.pass_names() == _renderer(soc).pass_names()
    assert _set_head(soc, r, kind, head_shadow) == 0
    assert _describe(r) == head
    assert lib.soc_renderer_set_terrain(r.handle, C.byref(_layer())) == 0
    assert lib.soc_renderer_set_draw_scene(r.handle, None, None, 0, 0, None) == 0
    assert "DrawTerrain" not in r.pass_names()
    rc, msg = _rc(soc, lib.soc_renderer_set_terrain, r.handle, C.byref(_layer()))
    assert rc == E_ARG and "head" in msg


def test_layer_leaves_draw_motion_alone(soc):
    """set_terrain rebuilds the graph but does not touch per-object motion; a shadow mesh of its own is kept."""
    lib = soc.lib()
    r = _renderer(soc)
    assert _set_head(soc, r, "draws", 1) == 0
    assert lib.soc_renderer_set_draw_motion(r.handle, 512) == 0
    assert lib.soc_debug_draw_motion(r.handle) == 1
    assert lib.soc_renderer_set_terrain(r.handle, C.byref(_layer(shadow_mesh=_mesh(normals=None, uvs=None)))) == 0
    assert lib.soc_debug_draw_motion(r.handle) == 1
    assert lib.soc_renderer_set_terrain(r.handle, None) == 0
    assert lib.soc_debug_draw_motion(r.handle) == 1
