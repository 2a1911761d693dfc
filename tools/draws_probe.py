#!/usr/bin/env python
"""What draw scenes cost (outside the benchmark): the C3 Sponza-proxy mesh at 3840x2160 rasterised three ways,

  mesh       through the single-mesh entry points (the baseline, same build);
  one_draw   as a draw scene of one draw;
  per_material  as one draw per material (25 draws, triangles sorted by material), each with its own transform;
  per_material_motion  the per_material scene resolved with per-object motion vectors (soc_gbuffer_resolve_draws_motion),
                its previous-transform array a separate copy equal to the current one (the resolve rows only: the
                visibility and shadow calls do not differ);

every transform holding the same (identity) matrix, so the three visibility buffers, shadow maps and G-buffers (and the
motion resolve's G-buffer) must be torch.equal: the probe asserts that before it times anything. Timed with device events around `--launches` calls,
`--rounds` times (the spread), after a warm-up of the same calls:

  vertex_setup_us   the raster's vertex stage alone: the call on a twin of the scene with the same vertices / slots and
                    no triangles (raster_setup or raster_setup_draws, nothing else is launched);
  visibility_us     the whole visibility call (clear + vertex stage + raster_small + raster_big);
  shadow_us         the whole 4096^2 depth-only call;
  resolve_us        the whole G-buffer resolve call (its vertex stage + the per-pixel kernel);
  resolve_vertex_plus_clear_us  the resolve on the triangle-free twin with an empty visibility buffer: its vertex stage
                    plus the per-pixel kernel writing clear values (the same in every form), so the differences between
                    the forms are the differences of the G-buffer vertex stage;
  build_us          soc_draw_scene_build (load time; host clock, it synchronises).

    python tools/draws_probe.py [--launches 50] [--rounds 5] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from soc_real_time_renderer_amd import raster  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--shadow", type=int, default=4096)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "draws_probe.py measures on the GPU"
    assert a.launches * a.rounds >= 20
    dev = torch.device("cuda", 0)
    W, H, S = a.width, a.height, a.shadow
    g, _gb, _sh, _nz, sc, _fr = bench.build_inputs("c3", "mesh", W, H, 0, dev)
    m = sc["host_mesh"]
    # one contiguous index range AND one contiguous vertex range per material (a vertex two materials share is stored
    # once per material), so a draw per material owns its vertices; all three forms read these arrays
    M = sc["material_count"]
    pos, nrm, uvs, tris, mats, vfirst, vcount = [], [], [], [], [], [], []
    base = 0
    for k in range(M):
        tk = m["indices"].reshape(-1, 3)[m["materials"] == k]
        uniq, inv = np.unique(tk, return_inverse=True)
        pos.append(m["positions"][uniq]); nrm.append(m["normals"][uniq]); uvs.append(m["uvs"][uniq])
        tris.append(inv.reshape(-1, 3).astype(np.int64) + base)
        mats.append(np.full(len(tk), k, np.uint32))
        vfirst.append(base); vcount.append(len(uniq))
        base += len(uniq)
    pos, nrm, uvs = np.concatenate(pos), np.concatenate(nrm), np.concatenate(uvs)
    tris = np.ascontiguousarray(np.concatenate(tris).astype(np.uint32))
    mats = np.concatenate(mats)
    V, T = len(pos), len(tris)
    mesh = raster.MeshBuffers.from_numpy(pos, nrm, uvs, tris, mats, device=dev)
    ws = mesh.workspace(dev)
    ident = np.eye(4, dtype=np.float32).reshape(1, 16)
    first = np.searchsorted(mats, np.arange(M))
    count = np.bincount(mats, minlength=M)
    forms = {"one_draw": None, "per_material": None}
    twins = {}
    build_us = {}
    for name in forms:
        if name == "one_draw":
            # one draw cannot carry 25 materials: its resolve is compared on material 0's pixels only (below)
            draws = [raster.draw(0, T, 0, V, transform=0, material=0)]
        else:
            draws = [raster.draw(3 * int(first[k]), int(count[k]), vfirst[k], vcount[k], transform=k, material=k)
                     for k in range(M)]
        n = len(draws)
        xf = raster.transforms_device(np.repeat(ident, n, 0), np.repeat(ident, n, 0), dev)
        forms[name] = raster.DrawScene(mesh.positions, mesh.normals, mesh.uvs, mesh.indices.reshape(-1), draws, xf,
                                       material_count=M, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        forms[name].build()                                      # a second build: the first loaded the kernels
        build_us[name] = round((time.perf_counter() - t0) * 1e6, 1)
        empty = [raster.draw(d.first_index, 0, d.first_vertex, d.vertex_count, d.transform, d.material) for d in draws]
        twins[name] = raster.DrawScene(mesh.positions, mesh.normals, mesh.uvs, mesh.indices.reshape(-1), empty, xf,
                                       material_count=M, device=dev)
    twin_mesh = raster.MeshBuffers(mesh.positions, mesh.normals, mesh.uvs, mesh.indices, mesh.materials)
    twin_mesh.struct.triangle_count = 0
    twin_ws = twin_mesh.workspace(dev)
    vp = np.ctypeslib.as_array(g.camera_projection_view_matrix)
    sun = np.ctypeslib.as_array(g.sun_info.projection_view_matrix)
    BC, BS = raster.SHADOW_BIAS_CONSTANT, raster.SHADOW_BIAS_SLOPE

    def images():
        o = {k: torch.zeros((H, W, 4), dtype=torch.float16, device=dev) for k in ("albedo", "emissive", "normal", "velocity")}
        o["depth"] = torch.zeros((H, W), dtype=torch.float32, device=dev)
        o["vis"] = torch.zeros((H, W), dtype=torch.int64, device=dev)
        o["shadow"] = torch.zeros((S, S), dtype=torch.float32, device=dev)
        return o

    def gb(o):
        return o["depth"], o["albedo"], o["emissive"], o["normal"], o["velocity"]
    out = {n: images() for n in ("mesh", "one_draw", "per_material", "per_material_motion")}
    previous = forms["per_material"].transforms.clone()          # previous == current, in memory of its own
    empty_vis = torch.zeros((H, W), dtype=torch.int64, device=dev)
    raster.raster_visibility(twin_mesh, vp, raster.CULL_FRONT, empty_vis, twin_ws)   # cleared, nothing drawn

    calls = {"mesh": {
        "vertex_setup_us": lambda: raster.raster_visibility(twin_mesh, vp, raster.CULL_FRONT, empty_vis, twin_ws, clear=False),
        "visibility_us": lambda: raster.raster_visibility(mesh, vp, raster.CULL_FRONT, out["mesh"]["vis"], ws),
        "shadow_us": lambda: raster.raster_depth(mesh, sun, raster.CULL_BACK, out["mesh"]["shadow"], ws, BC, BS),
        "resolve_us": lambda: raster.gbuffer_resolve(g, mesh, sc["materials"], M, out["mesh"]["vis"], *gb(out["mesh"]), ws),
        "resolve_vertex_plus_clear_us": lambda: raster.gbuffer_resolve(g, twin_mesh, sc["materials"], M, empty_vis,
                                                                       *gb(out["mesh"]), twin_ws)}}
    for name in forms:
        ds, tw, o = forms[name], twins[name], out[name]
        calls[name] = {
            "vertex_setup_us": lambda tw=tw: raster.raster_visibility_draws(tw, vp, raster.CULL_FRONT, empty_vis, clear=False),
            "visibility_us": lambda ds=ds, o=o: raster.raster_visibility_draws(ds, vp, raster.CULL_FRONT, o["vis"]),
            "shadow_us": lambda ds=ds, o=o: raster.raster_depth_draws(ds, sun, raster.CULL_BACK, o["shadow"], BC, BS),
            "resolve_us": lambda ds=ds, o=o: raster.gbuffer_resolve_draws(g, ds, sc["materials"], M, o["vis"], *gb(o)),
            "resolve_vertex_plus_clear_us": lambda tw=tw, o=o: raster.gbuffer_resolve_draws(g, tw, sc["materials"], M,
                                                                                            empty_vis, *gb(o))}

    pm, pm_twin, mo = forms["per_material"], twins["per_material"], out["per_material_motion"]
    calls["per_material_motion"] = {
        "resolve_us": lambda: raster.gbuffer_resolve_draws_motion(g, pm, previous, sc["materials"], M,
                                                                  out["per_material"]["vis"], *gb(mo)),
        "resolve_vertex_plus_clear_us": lambda: raster.gbuffer_resolve_draws_motion(g, pm_twin, previous, sc["materials"], M,
                                                                                    empty_vis, *gb(mo))}

    # ---- the forms give the same images
    for name in calls:
        for k in ("visibility_us", "shadow_us", "resolve_us"):
            if k in calls[name]:
                calls[name][k]()
    torch.cuda.synchronize()
    ref = out["mesh"]
    covered = (ref["vis"] & 0xFFFFFFFF) != 0xFFFFFFFF
    res = {"width": W, "height": H, "shadow": S, "vertices": V, "triangles": T, "materials": M,
           "covered": round(float(covered.float().mean()), 4), "build_us": build_us}
    for k in ("vis", "shadow", "depth", "albedo", "emissive", "normal", "velocity"):
        assert torch.equal(out["per_material"][k], ref[k]), ("per_material", k)
    for k in ("depth", "albedo", "emissive", "normal", "velocity"):
        assert torch.equal(mo[k], ref[k]), ("per_material_motion", k)
    for k in ("vis", "shadow", "depth", "velocity"):        # what does not depend on the material
        assert torch.equal(out["one_draw"][k], ref[k]), ("one_draw", k)
    mat0 = covered & (torch.from_numpy(mats.astype(np.int64)).to(dev)[(0xFFFFFFFE - (ref["vis"] & 0xFFFFFFFF)).clamp(0, T - 1)] == 0)
    for k in ("albedo", "emissive", "normal"):
        assert torch.equal(out["one_draw"][k][mat0], ref[k][mat0]), ("one_draw", k)
    res["identical"] = True
    print(json.dumps(res), flush=True)

    # ---- timings
    def timed(fn):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        us = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us.append(round(e0.elapsed_time(e1) / a.launches * 1e3, 2))
        return us
    res["us"] = {}
    for k in ("vertex_setup_us", "visibility_us", "shadow_us", "resolve_us", "resolve_vertex_plus_clear_us"):
        for name in ("mesh", "one_draw", "per_material", "per_material_motion", "mesh"):   # the baseline twice: its own spread
            if k not in calls[name]:
                continue
            key = name if name not in res["us"] or k not in res["us"][name] else name + "_again"
            res["us"].setdefault(key, {})[k] = timed(calls[name][k])
        print(k, {n: res["us"][n][k] for n in res["us"] if k in res["us"][n]}, flush=True)
    med = lambda v: float(np.median(v))   # noqa: E731
    res["ratio_to_mesh"] = {n: {k: round(med(res["us"][n][k]) / med(res["us"]["mesh"][k]), 3) for k in res["us"][n]}
                            for n in ("one_draw", "per_material", "per_material_motion", "mesh_again")}
    res["motion_to_per_material"] = {k: round(med(v) / med(res["us"]["per_material"][k]), 3)
                                     for k, v in res["us"]["per_material_motion"].items()}
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
