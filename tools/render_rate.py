#!/usr/bin/env python3
"""What a rendered frame costs (snk_render through DeviceVecEnv.render's path: device buffers, nothing leaves the GPU):
  (a) 4096 envs x 128 x 96 in ONE call, after a few gait env-steps (snakes spread over their worlds),
  (b) one env at 960 x 720, the size the reference renders (ppo/params.py's render_width / render_height),
each without and with SNK_RENDER_SHADOW, under the camera the reference sets (snake.py:322-325).  Beside each, in the same
session: the time of zeroing the same rgba + depth + segmentation buffers -- torch's zero_() on each of the three tensors, i.e.
three fill kernels, not hipMemsetAsync itself: the floor the output bytes alone set, as a kernel writes them.  Device events around `--reps` back-to-back calls after `--warmup` calls; `--rounds`
alternations of render and fill so that drift on the box falls on both alike.  Nothing is gated.
    python tools/render_rate.py [--reps 20] [--warmup 3] [--rounds 3]
Prints one JSON line per workload."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = (("4096 envs x 128x96", 4096, 128, 96), ("1 env x 960x720", 1, 960, 720))


def timed(torch, fn, reps, warmup):
    """ms per call of fn, from device events around `reps` calls."""
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import torch
    import bench
    pkg = importlib.import_module("bullet-envs_amd")
    lib = importlib.import_module("bullet-envs_amd._lib")
    if not torch.cuda.is_available():
        raise SystemExit("render_rate.py: no GPU (a rate is only measured on the device)")
    for name, envs, W, H in WORKLOADS:
        env = pkg.DeviceVecEnv(envs, n_modules=16)
        env.reset()
        for j in range(4):
            env.step(torch.from_numpy(bench.gait_actions(np.arange(envs), j, env.act_dim).astype(np.float32)).cuda())
        view, proj = lib.default_camera(W, H)
        cams = torch.as_tensor(np.concatenate([view, proj])[None], device=env.device)
        rgba = torch.empty((envs, H, W, 4), dtype=torch.uint8, device=env.device)
        dep = torch.empty((envs, H, W), dtype=torch.float32, device=env.device)
        seg = torch.empty((envs, H, W), dtype=torch.int32, device=env.device)
        st = torch.cuda.current_stream(env.device).cuda_stream

        def render(flags):
            env.stepper.render_device(0, envs, cams.data_ptr(), True, W, H, flags, rgba.data_ptr(), dep.data_ptr(),
                                      seg.data_ptr(), st)

        def fill():
            rgba.zero_(); dep.zero_(); seg.zero_()
        ms = {"plain": [], "shadow": [], "fill": []}
        for _ in range(a.rounds):
            ms["plain"].append(timed(torch, lambda: render(0), a.reps, a.warmup))
            ms["fill"].append(timed(torch, fill, a.reps, a.warmup))
            ms["shadow"].append(timed(torch, lambda: render(lib.RENDER_SHADOW), a.reps, a.warmup))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        drawn = float((seg > 0).float().mean())
        env.close()
        print(json.dumps(dict(
            workload=name, frames_per_call=envs, output_MB=round(envs * W * H * 12 / 1e6, 2),
            ms_per_call={k: [round(x, 4) for x in v] for k, v in ms.items()}, median_ms={k: round(v, 4) for k, v in med.items()},
            frames_per_s={k: round(envs / (med[k] * 1e-3), 1) for k in ("plain", "shadow")},
            over_fill_floor={k: round(med[k] / med["fill"], 2) for k in ("plain", "shadow")},
            share_of_pixels_on_the_snake=round(drawn, 4))), flush=True)


if __name__ == "__main__":
    main()
