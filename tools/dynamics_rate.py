#!/usr/bin/env python3
"""What the dynamics queries cost (DeviceWorld.dynamics / bias_forces / jacobians: snk_dynamics, snk_jacobians, outputs
resident on the device): ms per call over every env of a handle after a few gait env-steps, at 4096 envs x 16 links and at
1024 envs x 32 links --
    M + h                      [E, nd, nd] + [E, nd] f32
    h alone                    [E, nd]
    J of the head link         [E, 1, 6, nd]     (the last OUTPUT_BODY, link row 3n + 1, a point off its COM)
    J of all 2n cylinder links [E, 2n, 6, nd]    (their COMs)
-- each beside torch's zero fill of the same tensors (fill kernels: the floor the output bytes alone set) and beside
snk_link_states on the same handle (the same record load and forward kinematics), in alternating rounds so that drift on
the box falls on all alike.  Device events around the timed calls after `--warmup` untimed ones.  Nothing is gated.
    python tools/dynamics_rate.py [--reps 20] [--warmup 3] [--rounds 5] [--out profiles/r22_dynamics_rate.txt]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_dynamics_rate.txt"))
    a = ap.parse_args()
    import torch
    import bench
    pkg = importlib.import_module("bullet-envs_amd")
    if not torch.cuda.is_available():
        raise SystemExit("dynamics_rate.py: no GPU (a rate is only measured on the device)")
    lines = []
    for E, n in ((4096, 16), (1024, 32)):
        env = pkg.DeviceVecEnv(E, n_modules=n)
        env.reset()
        for j in range(4):
            env.step(torch.from_numpy(bench.gait_actions(np.arange(E), j, n // 2).astype(np.float32)).cuda())
        world = env.world
        dev = world.device
        head = torch.tensor([3 * n + 1], dtype=torch.int32, device=dev)
        head_pt = torch.tensor([[0.0, 0.0, 0.05]], dtype=torch.float32, device=dev)
        cyl = torch.tensor(sorted([3 * k - 1 for k in range(1, n + 1)] + [3 * k + 1 for k in range(1, n + 1)]),
                           dtype=torch.int32, device=dev)
        Mh = world.dynamics()
        Jhead = world.jacobians(head, head_pt)
        Jcyl = world.jacobians(cyl)
        ls = world.link_states()
        torch.cuda.synchronize()
        what = {
            "mass_and_bias": (lambda: world.dynamics(out=Mh), list(Mh)),
            "bias_alone": (lambda: world.bias_forces(out=Mh[1]), [Mh[1]]),
            "jacobian_head": (lambda: world.jacobians(head, head_pt, out=Jhead), [Jhead]),
            "jacobians_cylinders": (lambda: world.jacobians(cyl, out=Jcyl), [Jcyl]),
            "link_states": (lambda: world.link_states(out=ls), [ls]),
        }
        ms = {k: [] for k in what}
        fills = {k: [] for k in what}
        for _ in range(a.rounds):
            for k, (call, outs) in what.items():
                ms[k].append(timed(torch, call, a.reps, a.warmup))
                fills[k].append(timed(torch, lambda: [t.zero_() for t in outs], a.reps, a.warmup))
        for k, (call, outs) in what.items():
            nbytes = sum(t.numel() * t.element_size() for t in outs)
            med, fmed = float(np.median(ms[k])), float(np.median(fills[k]))
            lines.append(json.dumps(dict(
                measurement=k, envs=E, links=n, nd=n + 6, output_MB=round(nbytes / 1e6, 3),
                ms_per_call=[round(x, 4) for x in ms[k]], fill_ms_per_call=[round(x, 4) for x in fills[k]],
                median_ms=round(med, 4), median_fill_ms=round(fmed, 4), over_fill_floor=round(med / fmed, 2),
                GB_per_s=round(nbytes / (med * 1e-3) / 1e9, 1))))
            print(lines[-1], flush=True)
        env.close()
    with open(a.out, "w") as f:
        f.write("# tools/dynamics_rate.py --reps %d --warmup %d --rounds %d\n" % (a.reps, a.warmup, a.rounds))
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
