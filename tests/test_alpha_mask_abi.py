"""Alpha-masked materials through the C ABI and the Python layer without a GPU: the material struct's layout (the cutoff
took padding, nothing moved), the new symbols, every host-side refusal of the four masked calls and of the renderer's
setter (all made before any HIP call), raster.material's alpha_mode and the three keys gltf.load gives every material."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from soc_real_time_renderer_amd import _abi, gltf, raster

MASKED_CALLS = ("soc_raster_visibility_masked", "soc_raster_depth_masked", "soc_raster_visibility_draws_masked",
                "soc_raster_depth_draws_masked")


class MaterialBefore(C.Structure):
    """soc_material as it was before the cutoff: `int32_t pad[2]` after has_emissive."""
    _fields_ = [("albedo", _abi.SocImg), ("emissive", _abi.SocImg), ("albedo_factor", C.c_float * 4),
                ("emissive_factor", C.c_float * 4), ("flags", C.c_int32), ("has_emissive", C.c_int32),
                ("pad", C.c_int32 * 2), ("normal_map", _abi.SocImg), ("normal_image", _abi.SocImg),
                ("max_anisotropy", C.c_float), ("pad2", C.c_int32), ("paired_texels", C.c_void_p)]


def test_material_layout_the_cutoff_took_padding(soc):
    lib = soc.lib()
    off = lambda f: lib.soc_abi_offsetof(b"soc_material", f.encode())   # noqa: E731
    assert lib.soc_abi_sizeof(b"soc_material") == C.sizeof(MaterialBefore) == C.sizeof(_abi.Material)
    assert off("alpha_cutoff") == MaterialBefore.pad.offset == _abi.Material.alpha_cutoff.offset
    assert off("pad") == MaterialBefore.pad.offset + 4 == _abi.Material.pad.offset
    for name, _ in MaterialBefore._fields_:
        if name != "pad":
            assert off(name) == getattr(MaterialBefore, name).offset == getattr(_abi.Material, name).offset, name
    assert lib.soc_abi_version() == 1
    assert _abi.MATERIAL_ALPHA_MASK == 32
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "soc_rt.h")).read()
    assert "#define SOC_MATERIAL_ALPHA_MASK 32" in header and "float alpha_cutoff;" in header


def test_new_symbols_exist_and_are_bound(soc):
    lib = soc.lib()
    for name in MASKED_CALLS + ("soc_renderer_set_alpha_mask",):
        assert name in _abi.FUNCTIONS and getattr(lib, name) is not None, name


VP = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(-1).tolist())
FAKE = 4096   # a non-null address nothing dereferences: every case below returns before the first HIP call


def _mesh(uvs=FAKE):
    m = _abi.Mesh()
    m.positions, m.normals, m.indices, m.uvs = FAKE, FAKE, FAKE, uvs
    m.vertex_count, m.triangle_count = 3, 1
    return m


def _depth_img():
    return _abi.SocImg(FAKE, 8, 8, 32, _abi.FMT_D32F)


def _refused(soc, rc, *words):
    msg = soc.lib().soc_last_error_string().decode()
    assert rc == _abi.SOC_E_INVALID_ARG, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


@pytest.mark.parametrize("case", ["null materials", "material_count 0", "negative material_count", "null uvs"])
def test_mesh_calls_refuse_before_any_hip_call(soc, case):
    lib = soc.lib()
    mats, count = (None, 2) if case == "null materials" else (FAKE, {"material_count 0": 0, "negative material_count": -1}.get(case, 2))
    mesh = _mesh(None if case == "null uvs" else FAKE)
    word = "uvs" if case == "null uvs" else "materials"
    rc = lib.soc_raster_visibility_masked(C.byref(mesh), VP, raster.CULL_FRONT, FAKE, 8, 8, 1, FAKE, mats, count, None)
    _refused(soc, rc, "soc_raster_visibility_masked", word)
    rc = lib.soc_raster_depth_masked(C.byref(mesh), VP, raster.CULL_BACK, 1.25, 1.75, _depth_img(), FAKE, mats, count, None)
    _refused(soc, rc, "soc_raster_depth_masked", word)


def test_mesh_calls_keep_their_twins_refusals(soc):
    lib = soc.lib()
    mesh = _mesh()
    rc = lib.soc_raster_visibility_masked(None, VP, raster.CULL_FRONT, FAKE, 8, 8, 1, FAKE, FAKE, 2, None)
    _refused(soc, rc, "soc_raster_visibility_masked", "null mesh")
    rc = lib.soc_raster_visibility_masked(C.byref(mesh), VP, 3, FAKE, 8, 8, 1, FAKE, FAKE, 2, None)
    _refused(soc, rc, "soc_raster_visibility_masked", "cull mode")
    rc = lib.soc_raster_visibility_masked(C.byref(mesh), VP, raster.CULL_FRONT, FAKE, 8, 8, 1, None, FAKE, 2, None)
    _refused(soc, rc, "soc_raster_visibility_masked", "null argument")
    rc = lib.soc_raster_depth_masked(C.byref(mesh), None, raster.CULL_BACK, 0.0, 0.0, _depth_img(), FAKE, FAKE, 2, None)
    _refused(soc, rc, "soc_raster_depth_masked", "null argument")
    bad = _abi.SocImg(FAKE, 8, 8, 32, _abi.FMT_RGBA16F)
    rc = lib.soc_raster_depth_masked(C.byref(mesh), VP, raster.CULL_BACK, 0.0, 0.0, bad, FAKE, FAKE, 2, None)
    assert rc != _abi.SOC_OK and "soc_raster_depth_masked" in lib.soc_last_error_string().decode()


def _scene(material_count=3, uvs=FAKE):
    sc = _abi.DrawSceneStruct()
    sc.positions, sc.normals, sc.indices, sc.transforms, sc.uvs = FAKE, FAKE, FAKE, FAKE, uvs
    sc.workspace = FAKE   # 256-byte aligned, never built
    arr = (_abi.Draw * 1)(raster.draw(0, 1, 0, 3, transform=0, material=material_count - 1))
    sc.draws, sc.draw_count = arr, 1
    sc.vertex_count, sc.index_count, sc.transform_count, sc.material_count = 3, 3, 1, material_count
    return sc, arr


@pytest.mark.parametrize("case", ["null materials", "material_count 0", "null uvs", "fewer materials than the scene's",
                                  "unbuilt workspace", "null scene"])
def test_draw_scene_calls_refuse_before_any_hip_call(soc, case):
    lib = soc.lib()
    sc, keep = _scene(uvs=None if case == "null uvs" else FAKE)
    mats, count, word = FAKE, 3, "materials"
    if case == "null materials":
        mats = None
    elif case == "material_count 0":
        count = 0
    elif case == "null uvs":
        word = "uvs"
    elif case == "fewer materials than the scene's":
        count, word = 2, "2 materials, the scene's draws name up to 3"
    elif case == "unbuilt workspace":
        word = "was not built"
    elif case == "null scene":
        word = "null scene"
    scene = None if case == "null scene" else C.byref(sc)
    rc = lib.soc_raster_visibility_draws_masked(scene, VP, raster.CULL_FRONT, FAKE, 8, 8, 1, mats, count, None)
    _refused(soc, rc, "soc_raster_visibility_draws_masked", word)
    rc = lib.soc_raster_depth_draws_masked(scene, VP, raster.CULL_BACK, 1.25, 1.75, _depth_img(), mats, count, None)
    _refused(soc, rc, "soc_raster_depth_draws_masked", word)


def test_setter_refuses_a_null_renderer(soc):
    rc = soc.lib().soc_renderer_set_alpha_mask(None, 1)
    _refused(soc, rc, "soc_renderer_set_alpha_mask", "null renderer")


def test_material_alpha_mode(soc):
    m = raster.material()
    assert not m.flags & raster.MATERIAL_ALPHA_MASK and m.alpha_cutoff == 0.0
    m = raster.material(alpha_mode="OPAQUE", alpha_cutoff=0.7)
    assert not m.flags & raster.MATERIAL_ALPHA_MASK
    m = raster.material(alpha_mode="MASK")
    assert m.flags & raster.MATERIAL_ALPHA_MASK and m.alpha_cutoff == 0.5
    m = raster.material(alpha_mode="MASK", alpha_cutoff=0.25, albedo_factor=(1, 1, 1, 0.5), flags=raster.MATERIAL_ZERO_VELOCITY)
    assert m.flags == raster.MATERIAL_ALPHA_MASK | raster.MATERIAL_ZERO_VELOCITY
    assert m.alpha_cutoff == 0.25 and m.albedo_factor[3] == 0.5
    for bad in ("BLEND", "mask", "", "CUTOUT"):
        with pytest.raises(ValueError, match="alpha_mode"):
            raster.material(alpha_mode=bad)


def test_gltf_reports_alpha_mode_cutoff_and_base_color_factor(soc, tmp_path):
    """A document with one MASK material (alphaCutoff 0.25, a baseColorFactor), one BLEND and one default: the three
    keys of each, and the soc_material built from them."""
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    idx = np.array([0, 1, 2], np.uint16)
    blob = pos.tobytes() + idx.tobytes() + b"\0\0"
    (tmp_path / "tri.bin").write_bytes(blob)
    prim = lambda m: {"attributes": {"POSITION": 0}, "indices": 1, "material": m}   # noqa: E731
    doc = {"asset": {"version": "2.0"}, "scenes": [{"nodes": [0]}], "nodes": [{"mesh": 0}],
           "meshes": [{"primitives": [prim(0), prim(1), prim(2)]}],
           "buffers": [{"uri": "tri.bin", "byteLength": len(blob)}],
           "bufferViews": [{"buffer": 0, "byteOffset": 0, "byteLength": 36}, {"buffer": 0, "byteOffset": 36, "byteLength": 6}],
           "accessors": [{"bufferView": 0, "componentType": 5126, "count": 3, "type": "VEC3"},
                         {"bufferView": 1, "componentType": 5123, "count": 3, "type": "SCALAR"}],
           "materials": [{"alphaMode": "MASK", "alphaCutoff": 0.25,
                          "pbrMetallicRoughness": {"baseColorFactor": [1.0, 0.5, 0.25, 0.75]}},
                         {"alphaMode": "BLEND"}, {}]}
    (tmp_path / "tri.gltf").write_text(json.dumps(doc))
    out = gltf.load(str(tmp_path / "tri.gltf"))
    a, b, c = out["material_list"]
    assert (a["alpha_mode"], a["alpha_cutoff"], a["base_color_factor"]) == ("MASK", 0.25, (1.0, 0.5, 0.25, 0.75))
    assert (b["alpha_mode"], b["alpha_cutoff"], b["base_color_factor"]) == ("BLEND", 0.5, (1.0, 1.0, 1.0, 1.0))
    assert (c["alpha_mode"], c["alpha_cutoff"], c["base_color_factor"]) == ("OPAQUE", 0.5, (1.0, 1.0, 1.0, 1.0))
    assert out["materials"].tolist() == [0, 1, 2]
    m = raster.material(albedo=a["albedo"], alpha_mode=a["alpha_mode"], alpha_cutoff=a["alpha_cutoff"],
                        albedo_factor=a["base_color_factor"])
    assert m.flags & raster.MATERIAL_ALPHA_MASK and m.alpha_cutoff == 0.25 and m.albedo_factor[3] == 0.75
    # BLEND is reported as it stands; the renderer has no such mode, so a caller renders it opaque
    with pytest.raises(ValueError):
        raster.material(alpha_mode=b["alpha_mode"])
    m = raster.material(alpha_mode="MASK" if b["alpha_mode"] == "MASK" else "OPAQUE", alpha_cutoff=b["alpha_cutoff"])
    assert not m.flags & raster.MATERIAL_ALPHA_MASK
    assert not raster.material(alpha_mode=c["alpha_mode"], alpha_cutoff=c["alpha_cutoff"]).flags & raster.MATERIAL_ALPHA_MASK
