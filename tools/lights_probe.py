#!/usr/bin/env python
"""What bounded lights and the per-wave light culling cost and buy (outside the benchmark): Composition alone on C3's
inputs at 3840x2160 with C3b's 128 point lights (bench.point_lights_c3b, fed through soc_scene_update), as the render
graph launches it (the fused composition + histogram call) on one frame's own intermediates (one renderer frame makes
the blurred AO, the clouds and the bloom output). Four cases:

  a  unbounded          soc_composition_luminance_histogram, today's call;
  b  bounded_r0         bounded, every range 0, no cull: the price of bounds that bound nothing;
  c  bounded_r4         bounded, every range --range (4.0), no cull: the window's price;
  d  bounded_r4_cull    as c with SOC_LIGHTS_CULL: what the culling buys.

(c) and (d) must be torch.equal and (b) must equal (a), as bit patterns (a NaN pixel of the mesh G-buffer's non-unit
normals is NaN in both): the probe asserts both before it times anything. It also reads the
per-wave counter once per case (the counting kernels, not timed): the lights the waves ran. Timed with device events
around `--launches` calls, `--rounds` times (the median and the spread), after a warm-up of the same calls, in
`--processes` fresh processes one after the other (this process starts them and never touches the GPU itself).

    python tools/lights_probe.py [--launches 20] [--rounds 7] [--processes 2] [--out FILE.json]
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

    assert torch.cuda.is_available(), "lights_probe.py measures on the GPU"
    dev = torch.device("cuda", 0)
    W, H = a.width, a.height
    g, _gb, _sh, _nz, _sc, fr = bench.build_inputs("c3b", a.scene, W, H, 0, dev)
    npl = int(g.point_light_count)
    r = soc.Renderer(fr)
    r.execute(g)                 # the frame's intermediates: ssao_blur, clouds, bloom_output, d_globals
    torch.cuda.synchronize()
    r.close()
    ins = [fr[k] for k in ("albedo", "bloom_output", "normal", "depth", "ssao_blur", "shadow", "clouds")]
    scratch = soc.histogram_scratch(dev)
    ae = soc.auto_exposure_buffer(dev)
    b0, b4 = soc.light_bounds_device_buffer(dev), soc.light_bounds_device_buffer(dev)
    soc.upload_light_bounds(soc.light_bounds(), b0)
    soc.upload_light_bounds(soc.light_bounds([a.range] * npl), b4)
    cases = {"a_unbounded": {}, "b_bounded_r0": dict(bounds=b0, cull=False),
             "c_bounded_r4": dict(bounds=b4, cull=False), "d_bounded_r4_cull": dict(bounds=b4, cull=True)}
    outs = {n: torch.zeros(H, W, 4, dtype=torch.float16, device=dev) for n in cases}

    def call(name, **extra):
        soc.composition_luminance_histogram(g, outs[name], *ins, ae, scratch, d_globals=fr["d_globals"], **cases[name], **extra)

    res = {"width": W, "height": H, "scene": a.scene, "point_lights": npl, "range": a.range, "lit_fraction":
           round(float((fr["depth"] != 1.0).float().mean()), 4)}
    counts = {}
    for name in cases:
        call(name)
        if cases[name]:
            n = torch.zeros(1, dtype=torch.int32, device=dev)
            call(name, shaded_pairs=n)
            counts[name] = int(n.cpu()[0])
    torch.cuda.synchronize()
    # compared as bit patterns: the mesh G-buffer's non-unit normals give NaN pixels (in every case alike), and NaN != NaN
    bits = {n: o.view(torch.int16) for n, o in outs.items()}
    res["nan_pixels"] = {n: int(torch.isnan(o).any(dim=2).sum()) for n, o in outs.items()}
    for x, y, what in (("c_bounded_r4", "d_bounded_r4_cull", "the cull changed the frame"),
                       ("a_unbounded", "b_bounded_r0", "unlimited ranges changed the frame")):
        differ = int((bits[x] != bits[y]).any(dim=2).sum())
        assert torch.equal(bits[x], bits[y]), f"{what}: {differ} pixels differ; NaN pixels {res['nan_pixels']}"
    res["c_equals_d"] = res["a_equals_b"] = True
    res["lights_run_per_wave_sum"] = counts
    res["cull_keeps"] = round(counts["d_bounded_r4_cull"] / max(counts["c_bounded_r4"], 1), 4)

    def timed(name):
        for _ in range(5):
            call(name)
        torch.cuda.synchronize()
        us = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                call(name)
            e1.record()
            torch.cuda.synchronize()
            us.append(round(e0.elapsed_time(e1) / a.launches * 1e3, 1))
        return us
    order = list(cases) + ["a_unbounded"]          # the baseline twice: its own spread
    res["us"] = {}
    for name in order:
        key = name if name not in res["us"] else name + "_again"
        res["us"][key] = timed(name)
    med = {k: float(np.median(v)) for k, v in res["us"].items()}
    res["median_us"] = med
    res["ratios"] = {"b_over_a": round(med["b_bounded_r0"] / med["a_unbounded"], 3),
                     "c_over_a": round(med["c_bounded_r4"] / med["a_unbounded"], 3),
                     "d_over_c": round(med["d_bounded_r4_cull"] / med["c_bounded_r4"], 3),
                     "d_over_a": round(med["d_bounded_r4_cull"] / med["a_unbounded"], 3),
                     "a_again_over_a": round(med["a_unbounded_again"] / med["a_unbounded"], 3)}
    print("LIGHTS_PROBE " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--processes", type=int, default=2)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--range", type=float, default=4.0)
    ap.add_argument("--scene", choices=("mesh", "boxes"), default="mesh")
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
            sys.exit(f"lights_probe: process {i} ended with {p.returncode}")
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("LIGHTS_PROBE ")][-1]
        runs.append(json.loads(line[len("LIGHTS_PROBE "):]))
        print(f"process {i}: {json.dumps(runs[-1])}", flush=True)
    out = {"processes": runs}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
