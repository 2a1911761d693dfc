"""Per-object motion vectors of draw scenes through the C ABI without a GPU: the new symbols, every host-side refusal of
soc_gbuffer_resolve_draws_motion (made before any HIP call: the pointers here are not device memory, reaching a launch
would not return an error code) and soc_renderer_set_draw_motion's effect on the render graph (built and inspected,
nothing is launched)."""
import ctypes as C
import os

import numpy as np

from soc_real_time_renderer_amd import _abi, raster
from test_draws_abi import _rc, _renderer, _scene, _uses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("soc_gbuffer_resolve_draws_motion", "soc_renderer_set_draw_motion")


def test_symbols_are_declared_exported_and_bound(soc):
    lib = soc.lib()
    header = open(os.path.join(ROOT, "include", "soc_rt.h")).read()
    for name in NEW:
        assert name + "(" in header
        assert name in _abi.FUNCTIONS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int32 or fn.restype is C.c_int, name
        assert len(fn.argtypes) == len(_abi.FUNCTIONS[name][1])
    # one more pointer than soc_gbuffer_resolve_draws, nothing else
    assert len(_abi.FUNCTIONS[NEW[0]][1]) == len(_abi.FUNCTIONS["soc_gbuffer_resolve_draws"][1]) + 1
    assert lib.soc_abi_version() == 1
    assert hasattr(raster, "gbuffer_resolve_draws_motion") and hasattr(soc.Renderer, "set_draw_motion")


def test_host_refusals_without_a_launch(soc):
    lib = soc.lib()
    E_ARG, E_SHAPE = _abi.SOC_E_INVALID_ARG, _abi.SOC_E_SHAPE
    name = NEW[0]
    ok = raster.draw(0, 10, 0, 30, transform=1, material=1)
    bad = raster.draw(3, 10, 0, 30)                                    # 3 + 30 > 30 indices
    g = soc.globals_defaults(64, 36)
    vis = np.zeros((36, 64), np.uint64)
    depth = soc.img(np.ones((36, 64), np.float32))
    im = [soc.img(np.zeros((36, 64, 4), np.float16)) for _ in range(4)]

    def call(sc, prev=512, mats=256, count=2, visibility=vis.ctypes.data, d=depth, images=im, gp=C.byref(g)):
        return _rc(soc, lib.soc_gbuffer_resolve_draws_motion, gp, sc, prev, mats, count, visibility, d, *images, None)
    # the refusal of its own: a NULL previous array, whatever the scene
    for sc in (C.byref(_scene([ok])), None):
        rc, msg = call(sc, prev=None)
        assert rc == E_ARG and name in msg and "previous_transforms" in msg, msg
    # the existing call's checks, under the new name
    rc, msg = call(None)
    assert rc == E_ARG and name in msg
    for fld in ("positions", "indices", "transforms", "workspace"):
        rc, msg = call(C.byref(_scene([ok], **{fld: None})))
        assert rc == E_ARG and name in msg, fld
    for fld in ("normals", "uvs"):
        rc, msg = call(C.byref(_scene([ok], **{fld: None})))
        assert rc == E_ARG and name in msg and "normals" in msg, fld
    rc, msg = call(C.byref(_scene([ok], workspace=4096 + 64)))
    assert rc == E_ARG and "aligned" in msg
    rc, msg = call(C.byref(_scene([ok, ok, bad])))
    assert rc == E_SHAPE and name in msg and "draw 2" in msg
    rc, msg = call(C.byref(_scene([raster.draw(0, 10, 0, 30, transform=2)])))
    assert rc == E_SHAPE and name in msg and "transform" in msg
    # a workspace that was never built (so neither changed nor failed: those records exist only after a build)
    rc, msg = call(C.byref(_scene([ok])))
    assert rc == E_ARG and name in msg and "not built" in msg
    # the same answers as the existing call for the same scenes
    for sc in (_scene([ok]), _scene([ok, ok, bad]), _scene([ok], uvs=None)):
        rc0 = lib.soc_gbuffer_resolve_draws(C.byref(g), C.byref(sc), 256, 2, vis.ctypes.data, depth, *im, None)
        assert call(C.byref(sc))[0] == rc0


def test_set_draw_motion_on_the_render_graph(soc):
    lib = soc.lib()
    E_ARG = _abi.SOC_E_INVALID_ARG
    ok = raster.draw(0, 10, 0, 30, transform=1, material=1)
    sc = _scene([ok])
    off, r = _renderer(soc), _renderer(soc)
    assert lib.soc_renderer_set_draw_scene(off.handle, C.byref(sc), 256, 2, 1, 256) == 0
    rc, msg = _rc(soc, lib.soc_renderer_set_draw_motion, None, 512)
    assert rc == E_ARG and NEW[1] in msg
    # before a scene (and with a single-mesh scene) it is an error, also for NULL
    for prev in (512, None):
        rc, msg = _rc(soc, lib.soc_renderer_set_draw_motion, r.handle, prev)
        assert rc == E_ARG and NEW[1] in msg and "draw scene" in msg
    rs = _abi.RasterScene()
    for f in ("positions", "normals", "uvs", "indices"):
        setattr(rs.mesh, f, 1)
    rs.mesh.vertex_count, rs.mesh.triangle_count = 3, 1
    rs.materials, rs.material_count, rs.shadow, rs.visibility, rs.workspace = 1, 1, 1, 1, 1
    assert lib.soc_renderer_set_raster_scene(r.handle, C.byref(rs)) == 0
    assert lib.soc_renderer_set_draw_motion(r.handle, 512) == E_ARG
    # with a draw scene: on and off leave names, groups, declared uses and lanes as they are
    assert lib.soc_renderer_set_draw_scene(r.handle, C.byref(sc), 256, 2, 1, 256) == 0
    assert not lib.soc_debug_draw_motion(r.handle)
    before = (_uses(r), [r.pass_lane(i) for i in range(len(r.pass_names()))])
    for prev, on in ((512, True), (None, False), (512, True)):
        assert lib.soc_renderer_set_draw_motion(r.handle, prev) == 0
        assert bool(lib.soc_debug_draw_motion(r.handle)) == on
        assert (_uses(r), [r.pass_lane(i) for i in range(len(r.pass_names()))]) == before
        assert _uses(r) == _uses(off)
        assert r.pass_uses(r.pass_names().index("GBufferGeneration")) == off.pass_uses(off.pass_names().index("GBufferGeneration"))
    # replacing or clearing the scene turns it off: by either setter, with a scene or with NULL
    resets = (lambda: lib.soc_renderer_set_draw_scene(r.handle, C.byref(sc), 256, 2, 0, 256),
              lambda: lib.soc_renderer_set_raster_scene(r.handle, C.byref(rs)),
              lambda: lib.soc_renderer_set_draw_scene(r.handle, None, None, 0, 0, None),
              lambda: lib.soc_renderer_set_raster_scene(r.handle, None))
    for reset in resets:
        assert lib.soc_renderer_set_draw_scene(r.handle, C.byref(sc), 256, 2, 1, 256) == 0
        assert lib.soc_renderer_set_draw_motion(r.handle, 512) == 0 and lib.soc_debug_draw_motion(r.handle)
        assert reset() == 0
        assert not lib.soc_debug_draw_motion(r.handle)
    # the Python methods: the keyword sets it after the scene, None and a new scene turn it off
    from types import SimpleNamespace
    ds = SimpleNamespace(struct=sc)
    r.set_draw_scene(ds, 256, 2, 256, motion=512)
    assert lib.soc_debug_draw_motion(r.handle) and r._motion == 512
    r.set_draw_motion(None)
    assert not lib.soc_debug_draw_motion(r.handle) and r._motion is None
    r.set_draw_motion(512)
    r.set_draw_scene(ds, 256, 2, 256)
    assert not lib.soc_debug_draw_motion(r.handle) and r._motion is None
    r.set_draw_scene(None, None, 0, None)
    try:
        r.set_draw_motion(512)
        raise AssertionError("set_draw_motion without a scene must raise")
    except soc.SocError as e:
        assert e.rc == E_ARG
