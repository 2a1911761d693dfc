#!/usr/bin/env python
"""What the terrain layer costs (outside the benchmark): at 3840x2160 with a 4096^2 shadow map, the C3 Sponza-proxy mesh
as the raster head and the C4 terrain (grid 100, level 3, under the same globals and camera) as the layer. --globals
picks whose camera and sun: C3's (default; the mesh covers the view and hides nearly every terrain fragment, and the
terrain lies outside the sun's frustum) or C4's (the terrain fills the view and the shadow map, the mesh little of them).

  draw_terrain_us              soc_draw_terrain over the head's G-buffer (clear + raster + vertex stage + layer resolve)
  sun_shadow_draw_terrain_us   soc_sun_shadow_draw_terrain over the head's shadow map (no clear, no bias), under the
                               probe's own sun: an orthographic one straight above the terrain (probe_sun)

and, in the same process, the terrain ALONE through the existing single-mesh calls:

  terrain_visibility_us        soc_raster_visibility of the terrain (clear + raster)
  terrain_resolve_us           soc_gbuffer_resolve of that buffer (vertex stage + resolve, five images)
  terrain_raster_depth_us      soc_raster_depth of the terrain, bias 0 / 0 (clear + raster)

The layer's calls are idempotent (a terrain fragment ties with itself and wins again; atomicMin of the same depths), so
every timed call does the first call's work. Before timing, the probe checks the layer against the existing calls: over
the head's images the winner pixels carry the terrain-alone resolve's albedo, normal and velocity, every other pixel and
the whole emissive image the head's. Timed with device events around `--launches` calls, `--rounds` times, after a
warm-up; `--processes` fresh child processes one after the other, the medians of each and of all reported.

    python tools/terrain_layer_probe.py [--launches 50] [--rounds 5] [--processes 2] [--out FILE.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

ROWS = ("draw_terrain_us", "sun_shadow_draw_terrain_us", "terrain_visibility_us", "terrain_resolve_us",
        "terrain_raster_depth_us")


def probe_sun(positions):
    """An orthographic sun straight above the terrain's bounding box, three quarters of its longer side wide. The bench
    configurations' own sun matrices leave this terrain outside their depth range (no texel of it reaches the shadow map),
    which would time the vertex and triangle setup only. orthoRH_NO maps the depth range to [-1, 1] and fragments with
    z < 0 are clipped (quirk Q1): the terrain sits in the far half of the range."""
    import ctypes as C

    import numpy as np

    import soc_real_time_renderer_amd as soc
    lib, fp = soc.lib(), C.POINTER(C.c_float)
    lo, hi = positions.min(0).astype(np.float64), positions.max(0).astype(np.float64)
    centre, half = (lo + hi) / 2, 0.375 * max(hi[0] - lo[0], hi[2] - lo[2])
    h = max(100.0, 4.0 * (hi[1] - lo[1]))
    v3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])   # noqa: E731
    V, P, PV = (C.c_float * 16)(), (C.c_float * 16)(), (C.c_float * 16)()
    lib.soc_mat4_look_at_rh(C.cast(V, fp), C.cast(v3(centre + [0.0, h, 0.0]), fp), C.cast(v3(centre), fp),
                            C.cast(v3([1.0, 0.0, 0.0]), fp))
    lib.soc_mat4_ortho_rh_no(C.cast(P, fp), -half, half, -half, half, 0.5, 1.5 * h)
    lib.soc_mat4_mul(C.cast(PV, fp), C.cast(P, fp), C.cast(V, fp))
    return np.array(list(PV), np.float32)


def measure(a):
    import numpy as np
    import torch

    import bench
    from soc_real_time_renderer_amd import raster, scene
    assert torch.cuda.is_available(), "terrain_layer_probe.py measures on the GPU"
    dev = torch.device("cuda", 0)
    W, H, S = a.width, a.height, a.shadow
    g, _gb, _sh, _nz, head, _fr = bench.build_inputs("c3", "mesh", W, H, 0, dev)
    del _gb, _sh, _fr
    if a.globals == "c4":   # the terrain configuration's camera and sun: the terrain fills the view, the mesh little of it
        from soc_real_time_renderer_amd import multi_gpu
        g = bench.make_globals(W, H, multi_gpu.terrain_camera_for_rank(0))
    ter = raster.scene_setup(g, scene.TERRAIN, tex_size=1024, device=dev)
    tmesh, tws = ter["mesh"], ter["workspace"]
    layer_ws, shadow_ws = tmesh.workspace(dev), tmesh.workspace(dev)
    vp = np.ctypeslib.as_array(g.camera_projection_view_matrix)
    sun = probe_sun(ter["host_mesh"]["positions"])

    def images():
        o = {k: torch.zeros((H, W, 4), dtype=torch.float16, device=dev) for k in ("albedo", "emissive", "normal", "velocity")}
        o["depth"] = torch.zeros((H, W), dtype=torch.float32, device=dev)
        o["vis"] = torch.zeros((H, W), dtype=torch.int64, device=dev)
        o["shadow"] = torch.zeros((S, S), dtype=torch.float32, device=dev)
        return o

    def gb(o):
        return o["depth"], o["albedo"], o["emissive"], o["normal"], o["velocity"]
    fr, alone = images(), images()
    raster.raster_visibility(head["mesh"], vp, raster.CULL_FRONT, fr["vis"], head["workspace"])
    raster.gbuffer_resolve(g, head["mesh"], head["materials"], head["material_count"], fr["vis"], *gb(fr), head["workspace"])
    raster.raster_depth(head["mesh"], sun, raster.CULL_BACK, fr["shadow"], head["workspace"], raster.SHADOW_BIAS_CONSTANT,
                        raster.SHADOW_BIAS_SLOPE)
    before = {k: fr[k].clone() for k in ("depth", "albedo", "emissive", "normal", "velocity", "shadow")}
    layer_vis = torch.zeros((H, W), dtype=torch.int64, device=dev)
    calls = {
        "draw_terrain_us": lambda: raster.draw_terrain(g, tmesh, ter["materials"], ter["material_count"], layer_vis, fr["depth"],
                                                       fr["albedo"], fr["normal"], fr["velocity"], layer_ws),
        "sun_shadow_draw_terrain_us": lambda: raster.sun_shadow_draw_terrain(tmesh, sun, fr["shadow"], shadow_ws),
        "terrain_visibility_us": lambda: raster.raster_visibility(tmesh, vp, raster.CULL_FRONT, alone["vis"], tws),
        "terrain_resolve_us": lambda: raster.gbuffer_resolve(g, tmesh, ter["materials"], ter["material_count"], alone["vis"],
                                                             *gb(alone), tws),
        "terrain_raster_depth_us": lambda: raster.raster_depth(tmesh, sun, raster.CULL_BACK, alone["shadow"], tws, 0.0, 0.0),
    }
    for k in ROWS:
        calls[k]()
    torch.cuda.synchronize()
    # ---- the layer against the existing calls
    assert torch.equal(layer_vis, alone["vis"])
    hit = (layer_vis & 0xFFFFFFFF) != 0xFFFFFFFF
    win = hit & (alone["depth"].view(torch.int32) <= before["depth"].view(torch.int32))   # depths >= +0: the bits order
    for k in ("depth", "albedo", "normal", "velocity"):
        assert torch.equal(fr[k][win], alone[k][win]) and torch.equal(fr[k][~win], before[k][~win]), k
    assert torch.equal(fr["emissive"], before["emissive"])
    assert torch.equal(fr["shadow"], torch.minimum(before["shadow"], alone["shadow"]))
    res = {"globals": a.globals, "width": W, "height": H, "shadow": S, "head_triangles": int(head["mesh"].struct.triangle_count),
           "terrain_vertices": int(tmesh.struct.vertex_count), "terrain_triangles": int(tmesh.struct.triangle_count),
           "head_covered": round(float(((fr["vis"] & 0xFFFFFFFF) != 0xFFFFFFFF).float().mean()), 4),
           "terrain_fragments": round(float(hit.float().mean()), 4), "terrain_wins": round(float(win.float().mean()), 4),
           "terrain_shadow_texels": round(float((alone["shadow"] < 1).float().mean()), 4),
           "terrain_shadow_nearer": round(float((alone["shadow"] < before["shadow"]).float().mean()), 4), "identical": True}

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
    res["us"] = {k: timed(calls[k]) for k in ROWS}
    res["median_us"] = {k: float(np.median(v)) for k, v in res["us"].items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--processes", type=int, default=2)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--shadow", type=int, default=4096)
    ap.add_argument("--globals", choices=("c3", "c4"), default="c3",
                    help="camera and sun of the bench configuration: c3 (the mesh hides nearly all of the terrain: the "
                         "layer's early-out side) or c4 (the terrain wins nearly everywhere it has fragments)")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a)), flush=True)
        return
    runs = []
    for _ in range(a.processes):   # fresh processes one after the other; this one never opens the GPU
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [x for x in sys.argv[1:] if x != "--child"],
                           stdout=subprocess.PIPE, text=True, timeout=600)
        if p.returncode != 0:
            sys.exit(f"terrain_layer_probe: a measuring process ended with status {p.returncode}")
        runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(json.dumps(runs[-1]["median_us"]), flush=True)
    med = {k: round(sorted(r["median_us"][k] for r in runs)[len(runs) // 2] if len(runs) % 2 else
                    sum(r["median_us"][k] for r in runs) / len(runs), 2) for k in ROWS}
    res = {"processes": runs, "median_us": med,
           "layer_to_alone": {"draw_terrain / (visibility + resolve)":
                              round(med["draw_terrain_us"] / (med["terrain_visibility_us"] + med["terrain_resolve_us"]), 3),
                              "sun_shadow_draw_terrain / raster_depth":
                              round(med["sun_shadow_draw_terrain_us"] / med["terrain_raster_depth_us"], 3)}}
    print(json.dumps(res["median_us"]), json.dumps(res["layer_to_alone"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
