#!/usr/bin/env python3
"""What the ray test costs (DeviceWorld.ray_test: snk_ray_test, rays and records resident on the device): ms per call over
every env of a handle after a few gait env-steps, at 4096 envs x 16 links and at 1024 envs x 32 links, with 64 and with
1024 rays per env -- a 3 m sensor sphere riding on the head (link row 1) -- once as one shared set and once as a set per
row.  Each beside torch's zero fill of the same record tensor (the floor the output bytes alone set), beside snk_render of
as many pixels per env (8 x 8 and 32 x 32 images, colour and depth, no segmentation, no shadow: the same table kernel and
the same traversal, shading instead of records), and beside snk_link_states on the same handle (the same forward
kinematics), in alternating rounds so that drift on the box falls on all alike.  Device events around the timed calls
after `--warmup` untimed ones.  Nothing is gated.
    python tools/rays_rate.py [--reps 10] [--warmup 2] [--rounds 3] [--out profiles/r20_rays_rate.txt]
Prints one JSON line per measurement and writes the same lines to --out."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.world_rate import timed      # noqa: E402  (ms per call from device events)


def sensor_sphere(count, length=3.0):
    """[count, 6] float32: rays from the parent's origin to `count` points spread evenly over a sphere (a Fibonacci spiral)"""
    k = np.arange(count) + 0.5
    z = 1.0 - 2.0 * k / count
    phi = np.pi * (1.0 + 5.0 ** 0.5) * k
    s = np.sqrt(1.0 - z * z)
    to = length * np.stack([s * np.cos(phi), s * np.sin(phi), z], -1)
    return np.concatenate([np.zeros_like(to), to], -1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_rays_rate.txt"))
    a = ap.parse_args()
    import torch
    import bench
    pkg = importlib.import_module("bullet-envs_amd")
    lib = importlib.import_module("bullet-envs_amd._lib")
    if not torch.cuda.is_available():
        raise SystemExit("rays_rate.py: no GPU (a rate is only measured on the device)")
    lines = []
    for E, n in ((4096, 16), (1024, 32)):
        env = pkg.DeviceVecEnv(E, n_modules=n, obstacle=1, obstacle_pos=[0.45, 0.3, 0.1])
        env.reset()
        for j in range(4):
            env.step(torch.from_numpy(bench.gait_actions(np.arange(E), j, n // 2).astype(np.float32)).cuda())
        world = env.world
        states = world.link_states()
        for R, side in ((64, 8), (1024, 32)):
            fan = torch.as_tensor(sensor_sphere(R), device=world.device)
            per_row = fan.expand(E, R, 6).contiguous()
            hits = world.ray_test(fan, parent_row=1)
            torch.cuda.synchronize()
            ids = hits[..., 7]
            met = dict(ground=float((ids == 0).float().mean()), snake=float(((ids >= 1) & (ids <= 2 * n)).float().mean()),
                       box=float((ids == 1 + 2 * n).float().mean()), nothing=float((ids < 0).float().mean()))
            # the render of as many pixels: the [U] default camera over the middle of the chain, outputs allocated once
            view, proj = lib.default_camera(side, side, target=(-0.5 * n / 16, 0.0, 0.0))
            cams = torch.as_tensor(np.concatenate([view, proj]).astype(np.float32), device=world.device)
            rgba = torch.empty((E, side, side, 4), dtype=torch.uint8, device=world.device)
            depth = torch.empty((E, side, side), dtype=torch.float32, device=world.device)
            st, stream = world.stepper, world._stream()

            def render():
                st.render_device(0, E, cams.data_ptr(), True, side, side, 0, rgba.data_ptr(), depth.data_ptr(), 0, stream)
            ms = {"ray_test_shared": [], "ray_test_per_row": [], "fill": [], "render": [], "link_states": []}
            for _ in range(a.rounds):
                ms["ray_test_shared"].append(timed(torch, lambda: world.ray_test(fan, parent_row=1, out=hits), a.reps, a.warmup))
                ms["ray_test_per_row"].append(timed(torch, lambda: world.ray_test(per_row, parent_row=1, out=hits), a.reps, a.warmup))
                ms["fill"].append(timed(torch, hits.zero_, a.reps, a.warmup))
                ms["render"].append(timed(torch, render, a.reps, a.warmup))
                ms["link_states"].append(timed(torch, lambda: world.link_states(out=states), a.reps, a.warmup))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            lines.append(json.dumps(dict(
                measurement="snk_ray_test", envs=E, links=n, rays_per_env=R, parent_row=1, render_image="%dx%d" % (side, side),
                met={k: round(v, 3) for k, v in met.items()}, output_MB=round(hits.numel() * 4 / 1e6, 2),
                ms_per_call={k: [round(x, 4) for x in v] for k, v in ms.items()},
                median_ms={k: round(v, 4) for k, v in med.items()},
                Mrays_per_s=dict(shared=round(E * R / med["ray_test_shared"] / 1e3, 1),
                                 per_row=round(E * R / med["ray_test_per_row"] / 1e3, 1)),
                over_fill_floor=round(med["ray_test_per_row"] / med["fill"], 2),
                over_render=round(med["ray_test_per_row"] / med["render"], 2),
                over_link_states=round(med["ray_test_per_row"] / med["link_states"], 2))))
            print(lines[-1], flush=True)
        env.close()
    with open(a.out, "w") as f:
        f.write("# tools/rays_rate.py --reps %d --warmup %d --rounds %d\n" % (a.reps, a.warmup, a.rounds))
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
