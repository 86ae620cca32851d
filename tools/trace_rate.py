#!/usr/bin/env python3
"""What test mode's per-substep telemetry costs, in env-steps/s of the bench gait on one GPU, one process:
  (a) snk_step                       DeviceVecEnv.step, everything in device memory
  (b) snk_step_traced                the same with a resident trace tensor (DeviceVecEnv.step(trace=t))
  (c) SnakeVecEnv(mode='test')       the host seam with infos, telemetry='replay' and telemetry='kernel'
at 4096 envs of 16 links and 1024 envs of 32 links.  (a) and (b) alternate, `--rounds` times each, so that drift on the
box falls on both alike; a device synchronise closes every timed region; every region is bounded by its step count and,
for the host seams, by `--budget` seconds as well (the replay makes up to 41 launches and 82 full-batch downloads per
env-step).  Sensor passes per env-step: a traced step runs one per physics substep (the mean substep count printed here);
the plain step's own count needs the profile build (tools/dbg/sensor_rate.py: 1.018, profiles/r08_sensor_rate.txt).
    python tools/trace_rate.py [--links 16 32] [--steps 100] [--warmup 10] [--rounds 3] [--host-steps 5] [--budget 60]
Prints one JSON line per chain."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ENVS = {16: 4096, 32: 1024}


def device_rate(pkg, torch, bench, n, envs, steps, warmup, traced):
    env = pkg.DeviceVecEnv(envs, n_modules=n)
    env.reset()
    A = env.act_dim
    acts = [torch.from_numpy(bench.gait_actions(np.arange(envs), j, A).astype(np.float32)).cuda()
            for j in range(warmup + steps)]
    trace = torch.empty(env.trace_shape(), dtype=torch.float32, device="cuda") if traced else None
    for j in range(warmup):
        env.step(acts[j], trace=trace)
    torch.cuda.synchronize()
    subs = 0
    t0 = time.perf_counter()
    for j in range(warmup, warmup + steps):
        env.step(acts[j], trace=trace)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    subs = float(env.substeps.float().mean())        # (of the last step)
    env.close()
    return envs * steps / dt, subs


def host_rate(pkg, bench, n, envs, steps, budget, telemetry):
    env = pkg.SnakeVecEnv(envs, n_modules=n, mode='test', telemetry=telemetry)
    env.reset()
    A = env.action_space.shape[0]
    env.step(bench.gait_actions(np.arange(envs), 0, A).astype(np.float32))       # first use: buffers, scratch handle
    done_steps, rows = 0, 0
    t0 = time.perf_counter()
    for j in range(1, 1 + steps):
        infos = env.step(bench.gait_actions(np.arange(envs), j, A).astype(np.float32))[3]
        done_steps += 1
        rows += int(env.last_substeps.sum())
        assert len(infos[0]['internal_observations']) == env.last_substeps[0]
        if time.perf_counter() - t0 > budget:
            break
    dt = time.perf_counter() - t0
    env.close()
    return envs * done_steps / dt, done_steps, rows / float(envs * done_steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--links", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=5)
    ap.add_argument("--budget", type=float, default=60.0, help="seconds per host-seam region at the most")
    a = ap.parse_args()
    import torch
    import bench
    pkg = importlib.import_module("bullet-envs_amd")
    if not torch.cuda.is_available():
        raise SystemExit("trace_rate.py: no GPU (a rate is only measured on the device)")
    for n in a.links:
        envs = ENVS.get(n, 1024)
        runs = {"snk_step": [], "snk_step_traced": []}
        subs = 0.0
        for _ in range(a.rounds):
            runs["snk_step"].append(device_rate(pkg, torch, bench, n, envs, a.steps, a.warmup, False)[0])
            r, subs = device_rate(pkg, torch, bench, n, envs, a.steps, a.warmup, True)
            runs["snk_step_traced"].append(r)
        med = {k: float(np.median(v)) for k, v in runs.items()}
        host = {}
        for tel in ("replay", "kernel"):
            r, k, rows = host_rate(pkg, bench, n, envs, a.host_steps, a.budget, tel)
            host[tel] = dict(env_steps_per_s=round(r, 1), env_steps_timed=k, rows_per_env_step=round(rows, 2))
        print(json.dumps(dict(
            links=n, envs=envs, steps=a.steps,
            env_steps_per_s={k: [round(x, 1) for x in v] for k, v in runs.items()},
            median={k: round(v, 1) for k, v in med.items()},
            traced_over_plain=round(med["snk_step_traced"] / med["snk_step"], 4),
            sensor_passes_per_env_step_traced=round(subs, 2),
            vec_env_test_mode=host,
            kernel_over_replay=round(host["kernel"]["env_steps_per_s"] / host["replay"]["env_steps_per_s"], 2))), flush=True)


if __name__ == "__main__":
    main()
