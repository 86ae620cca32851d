#!/usr/bin/env python3
"""What the tensor seam costs (DeviceWorld's path: device buffers, nothing leaves the GPU), at 4096 envs x 16 links after
a few gait env-steps:
  (a) ms per snk_link_states call over every env ([4096, 50, 16] f32 = 13 MB), beside zeroing the same buffer (torch's
      zero_(): a fill kernel, the floor the output bytes alone set), in alternating rounds so that drift on the box falls
      on both alike;
  (b) env-steps/s of Snake.step's servo loop (snake.py:283-304) written in torch over snk_substep + snk_observe -- one
      masked single-substep launch, one observation / mean-height launch and a handful of torch element-wise kernels per
      pass -- beside snk_step on the same actions from the same start.  Two forms of the loop: `fixed` runs all
      max_counter + 1 passes (late passes find every env masked out) and never reads anything back; `early` reads one
      flag per pass and stops when no env is left inside its loop.  The loop has no reward / termination / reset (those
      would be a few more torch kernels), so after a `done` of the fused kernel the two populations differ: this is a
      rate, not a parity check (tests/test_gpu_world.py has that).
Device events around the timed calls after `--warmup` untimed ones.  Nothing is gated.
    python tools/world_rate.py [--envs 4096] [--reps 20] [--warmup 3] [--rounds 3] [--steps 10] [--out profiles/r14_world_rate.txt]
Prints one JSON line per measurement and writes the same lines to --out."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def servo_step(torch, world, action, obs, height, early):
    """One env-step of every env: the loop of snake.py:283-304 on tensors.  Returns the substep counts [E] int32."""
    P, n = world.params, world.n
    targets = torch.zeros((world.num_envs, n), dtype=torch.float32, device=world.device)
    targets[:, 1::2] = action.clamp(-1.0, 1.0) * float(np.float32(P.scaling_factor))
    t64 = targets.double()
    counter = torch.zeros(world.num_envs, dtype=torch.int32, device=world.device)
    world.observation(out=obs)
    active = (t64 - obs[:, :n].double()).norm(dim=1) > P.servo_tol
    for _ in range(P.max_counter + 1):
        if early and not bool(active.any()):
            break
        world.step_simulation(targets, 1, active=active)
        world.observation(out=obs)
        world.mean_height(out=height)
        counter += active.to(torch.int32)
        wants = (t64 - obs[:, :n].double()).norm(dim=1) > P.servo_tol
        active = active & wants & ~(height > P.height_threshold) & ~(counter > P.max_counter)
    return counter


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_world_rate.txt"))
    a = ap.parse_args()
    import torch
    import bench
    pkg = importlib.import_module("bullet-envs_amd")
    if not torch.cuda.is_available():
        raise SystemExit("world_rate.py: no GPU (a rate is only measured on the device)")
    E, n = a.envs, 16
    lines = []

    def report(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    def actions(j):
        return torch.from_numpy(bench.gait_actions(np.arange(E), j, n // 2).astype(np.float32)).cuda()

    env = pkg.DeviceVecEnv(E, n_modules=n)
    env.reset()
    for j in range(4):
        env.step(actions(j))
    torch.cuda.synchronize()
    start = env.stepper.snapshot()
    world = env.world

    # (a) link states of every env, beside a fill of the same bytes
    rows = torch.empty((E, world.link_rows, 16), dtype=torch.float32, device=env.device)
    ms = {"link_states": [], "fill": []}
    for _ in range(a.rounds):
        ms["link_states"].append(timed(torch, lambda: world.link_states(out=rows), a.reps, a.warmup))
        ms["fill"].append(timed(torch, rows.zero_, a.reps, a.warmup))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    report(measurement="snk_link_states", envs=E, links=world.link_rows, output_MB=round(rows.numel() * 4 / 1e6, 2),
           ms_per_call={k: [round(x, 4) for x in v] for k, v in ms.items()}, median_ms={k: round(v, 4) for k, v in med.items()},
           over_fill_floor=round(med["link_states"] / med["fill"], 2),
           GB_per_s=round(rows.numel() * 4 / (med["link_states"] * 1e-3) / 1e9, 1))

    # (b) the servo loop in torch over the seam, beside the fused step, each from `start` on the same actions
    obs = torch.empty((E, env.obs_dim), dtype=torch.float32, device=env.device)
    height = torch.empty(E, dtype=torch.float32, device=env.device)
    acts = [actions(4 + j) for j in range(a.warmup + a.steps)]
    res = {}
    for form in ("fused", "fixed", "early"):
        per_round, subs = [], 0.0
        for _ in range(a.rounds):
            env.stepper.restore(start)
            it = iter(acts)

            def one():
                if form == "fused":
                    env.step(next(it).clone())
                    return env.substeps
                return servo_step(torch, world, next(it), obs, height, form == "early")
            for _ in range(a.warmup):
                one()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            total = torch.zeros((), dtype=torch.float64, device=env.device)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.steps):
                total += one().sum()
            e1.record()
            e1.synchronize()
            per_round.append(e0.elapsed_time(e1) / a.steps)
            subs = float(total) / (a.steps * E)
        res[form] = float(np.median(per_round))
        report(measurement="env-step: " + {"fused": "snk_step", "fixed": "torch loop over snk_substep + snk_observe, all %d passes" % (env.params.max_counter + 1),
                                           "early": "torch loop over snk_substep + snk_observe, one flag read back per pass"}[form],
               envs=E, env_steps_timed=a.steps, ms_per_env_step=[round(x, 3) for x in per_round],
               median_ms=round(res[form], 3), env_steps_per_s=round(E / (res[form] * 1e-3), 1),
               mean_substeps_per_env_step=round(subs, 2))
    report(measurement="ratio", fused_over_fixed=round(res["fixed"] / res["fused"], 2), fused_over_early=round(res["early"] / res["fused"], 2),
           note="how many times the fused kernel's rate each torch loop costs")
    env.close()
    with open(a.out, "w") as f:
        f.write("# tools/world_rate.py --envs %d --reps %d --warmup %d --rounds %d --steps %d\n" % (E, a.reps, a.warmup, a.rounds, a.steps))
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
