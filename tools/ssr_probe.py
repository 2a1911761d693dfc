#!/usr/bin/env python
"""ScreenSpaceReflection probe on the bench's C3 inputs (the Sponza-proxy mesh at 3840x2160) with the tests' metallic
pattern (tests/ssr_oracle.py: a quarter of the pixels are copies, in 8x8 blocks):

* the kernel alone: warm-up, then device events around `--launches` launches, `--rounds` times (the spread);
* its divergence, from the `steps` image: the mean steps per marching pixel, the mean over the waves (8x8-pixel tiles)
  of the wave's largest step count, and their ratio (what a wave pays against what its lanes need: the lever for
  compacting the marching pixels);
* the bench's C3 frame (the same renderer settings as bench.py's default) without the pass, with it on the main lane and
  with it on the second lane: frames/sec over `--steps` frames, the three variants alternating `--rounds` times, and the
  pass's own milliseconds in the frame from its timing events (a separate, shorter run).

    python tools/ssr_probe.py [--steps 300] [--launches 200] [--rounds 3] [--out FILE.json]
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
import soc_real_time_renderer_amd as soc  # noqa: E402
from soc_real_time_renderer_amd import multi_gpu  # noqa: E402
from ssr_oracle import metallic_roughness_pattern  # noqa: E402


def divergence(steps: np.ndarray) -> dict:
    """Step statistics of a `steps` image over its 8x8-pixel waves (copies run no march: 0 steps)."""
    H, W = steps.shape
    marching = steps != 255
    n = np.where(marching, steps, 0).astype(np.int64)
    hp, wp = -(-H // 8) * 8, -(-W // 8) * 8
    pad = np.zeros((hp, wp), np.int64)
    pad[:H, :W] = n
    live = np.zeros((hp, wp), bool)
    live[:H, :W] = marching
    tiles = pad.reshape(hp // 8, 8, wp // 8, 8)
    wave_max = tiles.max(axis=(1, 3))
    wave_live = live.reshape(hp // 8, 8, wp // 8, 8).any(axis=(1, 3))
    mean_px = float(n[marching].mean())
    mean_wave = float(wave_max[wave_live].mean())
    return {"marching_share": float(marching.mean()), "miss_share": float((steps == 50).mean()),
            "hit_share": float((steps < 50).mean()), "mean_steps_per_marching_pixel": mean_px,
            "mean_wave_max_steps": mean_wave, "divergence_ratio": mean_wave / mean_px}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ssr_probe.py measures on the GPU"
    dev = torch.device("cuda", 0)
    W, H = a.width, a.height
    g, _gb, _sh, _nz, _sc, fr = bench.build_inputs("c3", "mesh", W, H, 0, dev)
    mr = torch.from_numpy(metallic_roughness_pattern(H, W)).to(dev)
    target = torch.zeros(H, W, 4, dtype=torch.float16, device=dev)
    steps = torch.zeros(H, W, dtype=torch.uint8, device=dev)
    res = {"width": W, "height": H}

    # ---- the kernel alone
    def alone(st):
        for _ in range(10):
            soc.screen_space_reflection(g, fr["depth"], fr["normal"], fr["albedo"], mr, target, st)
        torch.cuda.synchronize()
        us = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                soc.screen_space_reflection(g, fr["depth"], fr["normal"], fr["albedo"], mr, target, st)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) / a.launches * 1e3)
        return us
    res["kernel_us"] = alone(None)
    res["kernel_with_steps_us"] = alone(steps)
    print(f"kernel alone: {res['kernel_us']} us; writing the steps image: {res['kernel_with_steps_us']} us", flush=True)
    res["divergence"] = divergence(steps.cpu().numpy())
    print("divergence:", json.dumps(res["divergence"]), flush=True)

    # ---- in the C3 frame (bench.py's default renderer settings)
    for hv in fr["history_velocity"]:
        hv.copy_(fr["velocity"])
    bins = fr["auto_exposure"][1:]

    def renderer(variant, timing=False):
        r = soc.Renderer(fr, static_inputs=True, velocity_slots=True, bloom_in_composition=True, sky_lane_queue="low")
        if variant != "none":
            r.add_screen_space_reflection(mr, target, async_compute=variant == "async")
        r.set_exposure_pixels(*multi_gpu.exposure_pixels(1, W, H))
        if timing:
            r.set_pass_timing(r.pass_names().index("ScreenSpaceReflection"), True)
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

    # one renderer at a time: the frame's clouds workspace belongs to the renderer that runs on it
    variants = ("none", "main", "async")
    res["frames_per_sec"] = {v: [] for v in variants}
    for k in range(a.rounds):
        for v in variants:
            r = renderer(v)
            res["frames_per_sec"][v].append(round(fps(r, a.steps, a.warmup), 2))
            torch.cuda.synchronize()
            r.close()
        print(f"round {k}: " + ", ".join(f"{v} {res['frames_per_sec'][v][-1]} fps" for v in variants), flush=True)
    res["pass_ms_in_frame"] = {}
    for v in ("main", "async"):
        r = renderer(v, timing=True)
        fps(r, min(a.steps, 200), 30)
        ms = {n: m for n, _, m, cnt in r.pass_stats() if cnt}
        res["pass_ms_in_frame"][v] = round(ms["ScreenSpaceReflection"], 4)
        r.close()
    print("pass ms in frame:", res["pass_ms_in_frame"], flush=True)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
