#!/usr/bin/env python3
"""What the closest-point query costs (DeviceWorld.closest_points: snk_closest_points, outputs resident on the device): ms
per call over every env of a handle after a few gait env-steps, at 4096 envs x 16 links and at 1024 envs x 32 links, at
three distances -- the handle's own breaking threshold (nothing passes the cull), 0.05 m (the neighbours across a joint)
and 0.5 m (every pair passes the broad phase) -- with max_pairs 64.  Each beside torch's zero fill of the same three
tensors (the floor the output bytes alone set), beside snk_link_states on the same handle (the same forward kinematics),
and beside the clearance-only form (DeviceWorld.clearance: the same kernel without its record stores), in alternating
rounds so that drift on the box falls on all alike.  Device events around the timed calls after `--warmup` untimed ones.
Nothing is gated.
    python tools/closest_rate.py [--reps 10] [--warmup 2] [--rounds 3] [--out profiles/r19_closest_rate.txt]
Prints one JSON line per measurement and writes the same lines to --out."""
import argparse
import ctypes as C
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-pairs", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_closest_rate.txt"))
    a = ap.parse_args()
    import torch
    import bench
    pkg = importlib.import_module("bullet-envs_amd")
    if not torch.cuda.is_available():
        raise SystemExit("closest_rate.py: no GPU (a rate is only measured on the device)")
    lines = []
    for E, n in ((4096, 16), (1024, 32)):
        env = pkg.DeviceVecEnv(E, n_modules=n, obstacle=1, obstacle_pos=[0.45, 0.3, 0.1])
        env.reset()
        for j in range(4):
            env.step(torch.from_numpy(bench.gait_actions(np.arange(E), j, n // 2).astype(np.float32)).cuda())
        world = env.world
        derived = (C.c_double * 6)()
        assert world.stepper.lib.snk_params_derived(C.byref(world.stepper.params), derived) == 0
        states = world.link_states()
        for name, D in (("breaking_threshold", float(np.float32(derived[0]))), ("0.05", 0.05), ("0.5", 0.5)):
            out = world.closest_points(D, max_pairs=a.max_pairs)
            torch.cuda.synchronize()
            found = out[2].double().mean(0).tolist()

            def fill():
                for t in out:
                    t.zero_()
            ms = {"closest_points": [], "fill": [], "clearance_only": [], "link_states": []}
            for _ in range(a.rounds):
                ms["closest_points"].append(timed(torch, lambda: world.closest_points(D, max_pairs=a.max_pairs, out=out),
                                                  a.reps, a.warmup))
                ms["fill"].append(timed(torch, fill, a.reps, a.warmup))
                ms["clearance_only"].append(timed(torch, lambda: world.clearance(D, out=out[1]), a.reps, a.warmup))
                ms["link_states"].append(timed(torch, lambda: world.link_states(out=states), a.reps, a.warmup))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            nbytes = sum(t.numel() * t.element_size() for t in out)
            lines.append(json.dumps(dict(
                measurement="snk_closest_points", envs=E, links=n, distance=name, max_pairs=a.max_pairs,
                slots=int(out[0].shape[1]), found_per_env=dict(box=round(found[0], 2), links=round(found[1], 2)),
                output_MB=round(nbytes / 1e6, 2), ms_per_call={k: [round(x, 4) for x in v] for k, v in ms.items()},
                median_ms={k: round(v, 4) for k, v in med.items()},
                over_fill_floor=round(med["closest_points"] / med["fill"], 2),
                over_link_states=round(med["closest_points"] / med["link_states"], 2))))
            print(lines[-1], flush=True)
        env.close()
    with open(a.out, "w") as f:
        f.write("# tools/closest_rate.py --reps %d --warmup %d --rounds %d --max-pairs %d\n"
                % (a.reps, a.warmup, a.rounds, a.max_pairs))
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
