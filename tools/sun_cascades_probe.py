#!/usr/bin/env python
"""What cascaded sun shadow maps cost (outside the benchmark): Composition alone on C4's inputs at 3840x2160, as the
render graph launches it (the fused composition + histogram call) on one frame's own intermediates (one renderer frame
makes the blurred AO, the clouds and the bloom output). Three cases:

  a  one_map          soc_composition_luminance_histogram with the 4096^2 map, today's call;
  b  cascaded_sun     cascaded with the one-cascade record of the sun itself and the same map: the price of the form
                      when it selects nothing;
  c  cascaded_4       cascaded, count 4, S = 2048 (the same 64 MiB as the 4096^2 map), fitted to 16 .. 104 units.

(b) goes through the fp64 position where (a) goes through the fp32 combined matrix, so it is not the same arithmetic: the
probe reports how many pixels differ as bit patterns and the largest difference, it does not assert equality.
It also times SunShadowDraw of the tessellated terrain: four slab draws at 2048^2 (raster.sun_shadow_draw_cascades)
against the one draw at 4096^2 with the sun's own matrix. Timed with device events around `--launches` calls, `--rounds`
times (the median and the spread), after a warm-up of the same calls, in `--processes` fresh processes one after the
other (this process starts them and never touches the GPU itself).

    python tools/sun_cascades_probe.py [--launches 20] [--rounds 7] [--processes 1] [--out FILE.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def child(a):
    import numpy as np
    import torch

    import bench
    import soc_real_time_renderer_amd as soc
    from soc_real_time_renderer_amd import raster, scene

    assert torch.cuda.is_available(), "sun_cascades_probe.py measures on the GPU"
    dev = torch.device("cuda", 0)
    W, H = a.width, a.height
    g, _gb, _sh, _nz, _sc, fr = bench.build_inputs("c4", "mesh", W, H, 0, dev)
    r = soc.Renderer(fr)
    r.execute(g)                 # the frame's intermediates: ssao_blur, clouds, bloom_output, d_globals
    torch.cuda.synchronize()
    r.close()
    sun = soc.sun_cascades_from_sun(g, 4096)
    rec = soc.sun_cascades_fit(g, 4, a.map_size, a.near, a.max_distance, 0.5)
    sc = raster.scene_setup(g, scene.TERRAIN, tex_size=1024, device=dev)
    atlas = soc.sun_cascade_atlas(rec, dev)
    raster.sun_shadow_draw_cascades(sc["mesh"], rec, atlas, sc["workspace"])
    torch.cuda.synchronize()
    head = [fr[k] for k in ("albedo", "bloom_output", "normal", "depth", "ssao_blur")]
    scratch = soc.histogram_scratch(dev)
    ae = soc.auto_exposure_buffer(dev)
    cases = {"a_one_map": (fr["shadow"], None), "b_cascaded_sun": (fr["shadow"], sun), "c_cascaded_4": (atlas, rec)}
    outs = {n: torch.zeros(H, W, 4, dtype=torch.float16, device=dev) for n in cases}

    def call(name):
        shadow, record = cases[name]
        soc.composition_luminance_histogram(g, outs[name], *head, shadow, fr["clouds"], ae, scratch,
                                            d_globals=fr["d_globals"], cascades=record)

    depth = fr["depth"]
    lit = depth != 1.0
    res = {"width": W, "height": H, "map_size": a.map_size, "near": a.near, "max_distance": a.max_distance,
           "lit_fraction": round(float(lit.float().mean()), 4),
           "exponential_factor": [round(float(rec.exponential_factor[k]), 1) for k in range(4)]}
    k = torch.zeros_like(depth, dtype=torch.int32)
    for i in range(3):
        k += (depth > float(np.float32(rec.split_depth[i]))).int()
    res["cascade_shares_of_lit"] = [round(float(((k == c) & lit).sum() / lit.sum()), 4) for c in range(4)]
    for name in cases:
        call(name)
    torch.cuda.synchronize()
    differ = (outs["a_one_map"].view(torch.int16) != outs["b_cascaded_sun"].view(torch.int16)).any(dim=2)
    res["b_differs_from_a_pixels"] = int(differ.sum())
    res["b_minus_a_max_abs"] = float((outs["a_one_map"].float() - outs["b_cascaded_sun"].float()).abs().nan_to_num().max())
    # C4's lit pixels all lie outside the sun's one 32-unit box (a clamped tap and an out-of-range depth: no sun at all)
    res["c_brighter_than_a_fraction_of_lit"] = round(float(((outs["c_cascaded_4"][..., 0] > outs["a_one_map"][..., 0]) & lit).sum()
                                                           / lit.sum()), 4)

    def timed(fn):
        for _ in range(5):
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
            us.append(round(e0.elapsed_time(e1) / a.launches * 1e3, 1))
        return us

    res["us"] = {}
    for name in list(cases) + ["a_one_map"]:          # the baseline twice: its own spread
        key = name if name not in res["us"] else name + "_again"
        res["us"][key] = timed(lambda: call(name))
    one = torch.ones((4096, 4096), dtype=torch.float32, device=dev)
    sun_pv = list(g.sun_info.projection_view_matrix)
    res["us"]["raster_one_4096"] = timed(lambda: raster.raster_depth(sc["mesh"], sun_pv, raster.CULL_BACK, one, sc["workspace"],
                                                                     raster.SHADOW_BIAS_CONSTANT, raster.SHADOW_BIAS_SLOPE))
    res["us"]["raster_four_2048"] = timed(lambda: raster.sun_shadow_draw_cascades(sc["mesh"], rec, atlas, sc["workspace"]))
    med = {n: float(np.median(v)) for n, v in res["us"].items()}
    res["median_us"] = med
    res["ratios"] = {"b_over_a": round(med["b_cascaded_sun"] / med["a_one_map"], 3),
                     "c_over_a": round(med["c_cascaded_4"] / med["a_one_map"], 3),
                     "a_again_over_a": round(med["a_one_map_again"] / med["a_one_map"], 3),
                     "raster_four_over_one": round(med["raster_four_2048"] / med["raster_one_4096"], 3)}
    print("SUN_CASCADES_PROBE " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--processes", type=int, default=1)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--map-size", type=int, default=2048)
    ap.add_argument("--near", type=float, default=16.0)
    ap.add_argument("--max-distance", type=float, default=104.0)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = []
    for i in range(a.processes):
        cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [x for x in sys.argv[1:] if x != "--child"]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(f"sun_cascades_probe: process {i} ended with {p.returncode}")
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("SUN_CASCADES_PROBE ")][-1]
        runs.append(json.loads(line[len("SUN_CASCADES_PROBE "):]))
        print(f"process {i}: {json.dumps(runs[-1])}", flush=True)
    out = {"processes": runs}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
