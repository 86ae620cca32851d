#!/usr/bin/env python3
"""What reading the contacts costs (DeviceWorld.contacts: snk_contacts, outputs resident on the device): ms per call over
every env of a handle after a few gait env-steps, at 4096 envs x 16 links ([4096, 128, 16] f32 = 33.6 MB of records) and
at 1024 envs x 32 links ([1024, 256, 16] f32 = 16.8 MB) -- beside torch's zero fill of the same three tensors (fill
kernels: the floor the output bytes alone set), in alternating rounds so that drift on the box falls on both alike, and
beside the force-only form (DeviceWorld.contact_forces: the same kernel without its record stores).
Device events around the timed calls after `--warmup` untimed ones.  Nothing is gated.
    python tools/contacts_rate.py [--reps 20] [--warmup 3] [--rounds 5] [--out profiles/r16_contacts_rate.txt]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_contacts_rate.txt"))
    a = ap.parse_args()
    import torch
    import bench
    pkg = importlib.import_module("bullet-envs_amd")
    if not torch.cuda.is_available():
        raise SystemExit("contacts_rate.py: no GPU (a rate is only measured on the device)")
    lines = []
    for E, n in ((4096, 16), (1024, 32)):
        env = pkg.DeviceVecEnv(E, n_modules=n)
        env.reset()
        for j in range(4):
            env.step(torch.from_numpy(bench.gait_actions(np.arange(E), j, n // 2).astype(np.float32)).cuda())
        world = env.world
        out = world.contacts()
        torch.cuda.synchronize()
        live = float(out[2].double().mean())

        def fill():
            for t in out:
                t.zero_()
        ms = {"contacts": [], "fill": [], "forces_only": []}
        for _ in range(a.rounds):
            ms["contacts"].append(timed(torch, lambda: world.contacts(out=out), a.reps, a.warmup))
            ms["fill"].append(timed(torch, fill, a.reps, a.warmup))
            ms["forces_only"].append(timed(torch, lambda: world.contact_forces(out=out[1]), a.reps, a.warmup))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        nbytes = sum(t.numel() * t.element_size() for t in out)
        lines.append(json.dumps(dict(
            measurement="snk_contacts", envs=E, links=n, slots=int(out[0].shape[1]), live_slots_per_env=round(live, 1),
            output_MB=round(nbytes / 1e6, 2), ms_per_call={k: [round(x, 4) for x in v] for k, v in ms.items()},
            median_ms={k: round(v, 4) for k, v in med.items()}, over_fill_floor=round(med["contacts"] / med["fill"], 2),
            GB_per_s=round(nbytes / (med["contacts"] * 1e-3) / 1e9, 1))))
        print(lines[-1], flush=True)
        env.close()
    with open(a.out, "w") as f:
        f.write("# tools/contacts_rate.py --reps %d --warmup %d --rounds %d\n" % (a.reps, a.warmup, a.rounds))
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
