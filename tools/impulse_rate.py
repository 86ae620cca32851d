#!/usr/bin/env python3
"""What applying forces costs (DeviceWorld.apply_forces / impulse_response: snk_apply_impulse, every buffer resident on the
device): ms per call over every env of a handle after a few gait env-steps, at 4096 envs x 16 links and at 1024 envs x 32
links --
    gen_force alone            [E, nd] f32 in
    one wrench                 [E, 1, 9] f32 in   (the head link, LINK_FRAME)
    2n wrenches                [E, 2n, 9] f32 in  (one per cylinder link)
-- each writing the state and DRY, beside snk_dynamics (M + h) on the same handle (the same record load and forward
kinematics, the query the parent measured in profiles/r22_dynamics_rate.txt) and beside torch's zero fill of delta (a fill
kernel: the floor a launch and the output bytes alone set), in alternating rounds so that drift on the box falls on all
alike.  Device events around the timed calls after `--warmup` untimed ones.  Then env-steps/s of the fused env-step
(DeviceVecEnv.step: snk_step) with one push on the head in front of every step against without, on the same actions.
Nothing is gated.
    python tools/impulse_rate.py [--reps 20] [--warmup 3] [--rounds 5] [--steps 30] [--out profiles/r25_impulse_rate.txt]
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
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_impulse_rate.txt"))
    a = ap.parse_args()
    import torch
    import bench
    pkg = importlib.import_module("bullet-envs_amd")
    if not torch.cuda.is_available():
        raise SystemExit("impulse_rate.py: no GPU (a rate is only measured on the device)")
    lines = []
    for E, n in ((4096, 16), (1024, 32)):
        env = pkg.DeviceVecEnv(E, n_modules=n)
        env.reset()
        actions = [torch.from_numpy(bench.gait_actions(np.arange(E), j, n // 2).astype(np.float32)).cuda() for j in range(8)]
        for j in range(4):
            env.step(actions[j])
        world = env.world
        dev = world.device
        nd = n + 6
        g = torch.Generator(device="cpu").manual_seed(n)
        gf = (torch.rand((E, nd), generator=g) - 0.5).to(dev)
        head = torch.tensor([3 * n + 1], dtype=torch.int32, device=dev)
        w1 = torch.zeros((E, 1, 9), dtype=torch.float32, device=dev)
        w1[:, 0, 1] = 1.0                                          # 1 N along the head's own y, at its COM
        cyl = torch.tensor(sorted([3 * k - 1 for k in range(1, n + 1)] + [3 * k + 1 for k in range(1, n + 1)]),
                           dtype=torch.int32, device=dev)
        wc = ((torch.rand((E, 2 * n, 9), generator=g) - 0.5) * 0.1).to(dev)
        delta = torch.zeros((E, nd), dtype=torch.float32, device=dev)
        Mh = world.dynamics()
        seconds = 1e-6                                             # (small: hundreds of timed pushes must not fling the snakes away)
        torch.cuda.synchronize()
        what = {}
        for name, args in (("gen_force", (gf, None, None)), ("one_wrench", (None, head, w1)), ("wrenches_2n", (None, cyl, wc))):
            for dry in (False, True):
                what[name + ("_dry" if dry else "")] = (
                    lambda args=args, dry=dry: world.apply_forces(*args, frame="link", duration=seconds, dry=dry, out=delta))
        what["mass_and_bias"] = lambda: world.dynamics(out=Mh)
        what["zero_fill_of_delta"] = lambda: delta.zero_()
        ms = {k: [] for k in what}
        for _ in range(a.rounds):
            for k, call in what.items():
                ms[k].append(timed(torch, call, a.reps, a.warmup))
        ref = float(np.median(ms["mass_and_bias"]))
        for k in what:
            med = float(np.median(ms[k]))
            lines.append(json.dumps(dict(measurement=k, envs=E, links=n, nd=nd, ms_per_call=[round(x, 4) for x in ms[k]],
                                         median_ms=round(med, 4), over_mass_and_bias=round(med / ref, 2))))
            print(lines[-1], flush=True)
        # the fused env-step with a push in front of every step, and without
        rates = {"step": [], "push_then_step": []}
        for _ in range(a.rounds):
            for k in rates:
                env.reset()

                def one(j=[0], k=k):
                    if k == "push_then_step":
                        world.apply_forces(None, head, w1, frame="link")
                    env.step(actions[j[0] % len(actions)])
                    j[0] += 1

                rates[k].append(E / (timed(torch, one, a.steps, a.warmup) * 1e-3))
        for k, v in rates.items():
            lines.append(json.dumps(dict(measurement="env_steps_per_s_" + k, envs=E, links=n, per_round=[round(x) for x in v],
                                         median=round(float(np.median(v))))))
            print(lines[-1], flush=True)
        env.close()
    with open(a.out, "w") as f:
        f.write("# tools/impulse_rate.py --reps %d --warmup %d --rounds %d --steps %d\n" % (a.reps, a.warmup, a.rounds, a.steps))
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
