#!/usr/bin/env python
"""Depth-of-field probe on the bench's C3 inputs (the Sponza-proxy mesh at 3840x2160):

* the chain (soc_depth_of_field_mips) alone, in the fused form and in the per-level baseline form
  (SOC_DOF_CHAIN_FUSED=0), with each form's launch count, and the pass (soc_depth_of_field) alone: warm-up, then device
  events around `--launches` calls, `--rounds` times (the spread); the colour is the C3 frame's own;
* the algorithmic bytes of both and the time they take at `--tbps` TB/s;
* the C3 frame on an unfused-histogram renderer (the pass needs one; otherwise bench.py's settings) without and with the
  pass pair: frames/sec over `--steps` frames, alternating `--rounds` times, and the two passes' own milliseconds in the
  frame from their timing events (a separate, shorter run).

    python tools/dof_probe.py [--steps 300] [--launches 200] [--rounds 3] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import bench  # noqa: E402
import soc_real_time_renderer_amd as soc  # noqa: E402
from soc_real_time_renderer_amd import multi_gpu  # noqa: E402

TAIL_TEXELS = 4096   # csrc/dof.hip kDofTailTexels


def chain_launches(shapes, fused):
    """Launches of soc_depth_of_field_mips for the level shapes [(h, w)] (the host logic of csrc/dof.hip)."""
    L = len(shapes)
    if not fused:
        return L
    h, w = shapes[0]
    k, n = (2, 1) if L > 1 and w % 2 == 0 and h % 2 == 0 else (1, 1)
    tail = L
    while tail > k and shapes[tail - 1][0] * shapes[tail - 1][1] <= TAIL_TEXELS:
        tail -= 1
    return n + (tail - k) + (1 if tail < L else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--tbps", type=float, default=6.3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "dof_probe.py measures on the GPU"
    dev = torch.device("cuda", 0)
    W, H = a.width, a.height
    g, _gb, _sh, _nz, _sc, fr = bench.build_inputs("c3", "mesh", W, H, 0, dev)
    for hv in fr["history_velocity"]:
        hv.copy_(fr["velocity"])
    bins = fr["auto_exposure"][1:]
    chain = soc.depth_of_field_chain(W, H, dev)
    shapes = chain.level_shapes()
    res = {"width": W, "height": H, "levels": len(shapes)}

    def renderer(with_pass, timing=False):
        r = soc.Renderer(fr, static_inputs=True, velocity_slots=True, fused_histogram=False, sky_lane_queue="low")
        if with_pass:
            r.add_depth_of_field(chain)
        r.set_exposure_pixels(*multi_gpu.exposure_pixels(1, W, H))
        if timing:
            for n in ("MipMapping", "DepthOfField"):
                r.set_pass_timing(r.pass_names().index(n), True)
        return r

    def fps(r, steps_, warmup):
        for _ in range(warmup):
            multi_gpu.render_frame(r, g, bins)
        torch.cuda.synchronize()
        r.reset_timing()
        t0 = time.perf_counter()
        for _ in range(steps_):
            multi_gpu.render_frame(r, g, bins)
        torch.cuda.synchronize()
        return steps_ / (time.perf_counter() - t0)

    # the frame's colour, as Composition leaves it
    r = renderer(False)
    fps(r, 2, 2)
    r.close()
    color = fr["color"].clone()
    target = torch.zeros_like(color)

    # ---- alone
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
    res["chain_us"], res["chain_launches"] = {}, {}
    for name, fused in (("per_level", 0), ("fused", 1), ("per_level_again", 0), ("fused_again", 1)):
        os.environ["SOC_DOF_CHAIN_FUSED"] = str(fused)
        soc.reload_tuning()
        res["chain_us"][name] = timed(lambda: soc.depth_of_field_mips(color, chain))
        res["chain_launches"][name] = chain_launches(shapes, fused)
    del os.environ["SOC_DOF_CHAIN_FUSED"]
    soc.reload_tuning()
    res["pass_us"] = timed(lambda: soc.depth_of_field(g, fr["depth"], chain, target))
    res["pass_in_place_us"] = timed(lambda: soc.depth_of_field(g, fr["depth"], chain, color))
    texels = [h * w for h, w in shapes]
    # the chain: read the colour, write level 0, write every further level once (their reads hit the cache);
    # the pass: read the depth (4 B) and the chain's taps once per texel of the levels (8 B), write the target (8 B)
    res["chain_bytes"] = 8 * (2 * texels[0] + sum(texels[1:]))
    res["pass_bytes"] = W * H * (4 + 8) + 8 * sum(texels)
    res["chain_floor_us"] = round(res["chain_bytes"] / (a.tbps * 1e12) * 1e6, 2)
    res["pass_floor_us"] = round(res["pass_bytes"] / (a.tbps * 1e12) * 1e6, 2)
    print(json.dumps({k: res[k] for k in ("chain_us", "chain_launches", "pass_us", "pass_in_place_us", "chain_bytes",
                                          "pass_bytes", "chain_floor_us", "pass_floor_us")}), flush=True)

    # ---- in the C3 frame
    res["frames_per_sec"] = {"none": [], "dof": []}
    for k in range(a.rounds):
        for name, with_pass in (("none", False), ("dof", True)):
            r = renderer(with_pass)
            res["frames_per_sec"][name].append(round(fps(r, a.steps, a.warmup), 2))
            torch.cuda.synchronize()
            r.close()
        print(f"round {k}: " + ", ".join(f"{v} {res['frames_per_sec'][v][-1]} fps" for v in res["frames_per_sec"]), flush=True)
    r = renderer(True, timing=True)
    fps(r, min(a.steps, 200), 30)
    ms = {n: m for n, _, m, cnt in r.pass_stats() if cnt}
    res["pass_ms_in_frame"] = {n: round(ms[n], 4) for n in ("MipMapping", "DepthOfField")}
    r.close()
    print("pass ms in frame:", res["pass_ms_in_frame"], flush=True)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
