#!/usr/bin/env python3
"""Env-steps/s of the bench gait under a solver-rules set against the defaults, 4096 envs per chain, on one GPU: the fused
env-step kernel through DeviceVecEnv (actions, observations, rewards and done flags in device memory; a device synchronise
closes every timed region).  The configurations are measured alternately, `--rounds` times each, so that drift on the
box falls on all of them alike.  bench.py keeps its own flags; this is where the rule sets are timed.
    python tools/rules_rate.py [--links 16 32] [--steps 100] [--warmup 10] [--rounds 3]
Prints one JSON line per chain: the rate of every round of every configuration, and the median per configuration."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    "default": dict(),
    "as-read": dict(noncontact_order=1, contact_order=2, contact_erp_rule=1),   # Bullet as read
}


def rate(pkg, torch, bench, n, over, envs, steps, warmup):
    env = pkg.DeviceVecEnv(envs, n_modules=n, **over)
    env.reset()
    A = env.act_dim
    acts = [torch.from_numpy(bench.gait_actions(np.arange(envs), j, A).astype(np.float32)).cuda()
            for j in range(warmup + steps)]
    for j in range(warmup):
        env.step(acts[j])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for j in range(warmup, warmup + steps):
        env.step(acts[j])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    env.close()
    return envs * steps / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--links", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import torch
    import bench
    pkg = importlib.import_module("bullet-envs_amd")
    if not torch.cuda.is_available():
        raise SystemExit("rules_rate.py: no GPU (a rate is only measured on the device)")
    for n in a.links:
        runs = {k: [] for k in CONFIGS}
        for _ in range(a.rounds):
            for name, over in CONFIGS.items():
                runs[name].append(rate(pkg, torch, bench, n, over, a.envs, a.steps, a.warmup))
        print(json.dumps(dict(links=n, envs=a.envs, steps=a.steps, configs=CONFIGS,
                              env_steps_per_s={k: [round(v, 1) for v in r] for k, r in runs.items()},
                              median={k: round(float(np.median(r)), 1) for k, r in runs.items()})), flush=True)


if __name__ == "__main__":
    main()
