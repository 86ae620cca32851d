"""The scenes of tests/test_np_render.py (CPU) and tests/test_gpu_render.py (GPU): handles, states, boxes, cameras and render
calls, generated from seeds, and the float64 model's / the float32 twin's images of each call, computed once per process.
Both files walk the same list, so the retention displacement (np_render.DELTA) determined on the CPU is the one the GPU
gates use, on the same pixels."""
import functools

import numpy as np

import np_render as R
from conftest import random_state

N_ENVS = 5
# kind -> (n_modules, snk_params overrides).  "16s": static box (register-resident kernels' LDS image); "16f": free box
# (streamed-row image), moved and rotated with snk_set_box; "32": no box
KINDS = {
    "16s": (16, dict(obstacle=1, obstacle_pos=[1.0, 0.62, 0.1])),
    "16f": (16, dict(obstacle=2)),
    "32": (32, dict()),
}
SIZES = {"full": (64, 48), "odd": (37, 23)}      # 37 x 23: partial tiles on both edges, rows that are no multiple of 16


def states(kind):
    """[N_ENVS, 13 + 2n] float32: env 0 at rest on the ground; 1 flat on the ground, bent; 2 folded joints, tumbling in the
    air; 3 lifted and rolled so that end caps face the cameras; 4 random.  Bases near x = 1.6: the chain runs towards -x,
    into the view of the reference's camera (target [1.28, 0, 0])."""
    n = KINDS[kind][0]
    rng = np.random.default_rng(1100 + n + len(kind))
    S = np.zeros((N_ENVS, 13 + 2 * n))
    S[:, 6] = 1.0
    S[1] = random_state(rng, n, z=0.0, qamp=0.5, flat=True)
    S[2] = random_state(rng, n, z=0.25, qamp=1.5)
    S[3] = random_state(rng, n, z=0.3, qamp=0.3)
    ang = 1.2                                          # the chain's axis (-x at rest) pitched up towards the cameras
    S[3, 3:7] = [0.3 * np.sin(ang / 2), np.sin(ang / 2) * 0.954, 0.0, np.cos(ang / 2)]
    S[3, 3:7] /= np.linalg.norm(S[3, 3:7])
    S[4] = random_state(rng, n, z=0.15, qamp=0.8)
    S[:, 0] += 1.6 if n == 16 else 2.2
    S[:, 7:13] = 0.0
    S[:, 13 + n:] = 0.0
    return S.astype(np.float32)


def boxes(kind):
    """None, or per env (centre, quaternion or None, half extents) as float32-rounded values; "16f": [N_ENVS, 13] states
    for snk_set_box come from box_states()."""
    n, over = KINDS[kind]
    if kind == "16s":
        return [(np.array(over["obstacle_pos"]), None, np.array([0.1, 0.4, 0.1]))] * N_ENVS
    if kind == "16f":
        B = box_states()
        return [(B[e, 0:3].astype(np.float64), B[e, 3:7].astype(np.float64), np.array([0.1, 0.4, 0.1])) for e in range(N_ENVS)]
    return [None] * N_ENVS


def box_states():
    B = np.zeros((N_ENVS, 13))
    for e in range(N_ENVS):
        az, axx = 0.3 * e + 0.2, 0.2 * e
        qz = np.array([0, 0, np.sin(az / 2), np.cos(az / 2)])
        qx = np.array([np.sin(axx / 2), 0, 0, np.cos(axx / 2)])
        x1, y1, z1, w1 = qz
        x2, y2, z2, w2 = qx
        q = np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                      w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2])
        B[e, 0:3] = [0.9 + 0.1 * e, 0.55, 0.1 + 0.03 * e]
        B[e, 3:7] = q / np.linalg.norm(q)
    return B.astype(np.float32)


def cameras(kind, aspect):
    """name -> (view16, proj16, near, far), float32-rounded (what the GPU is handed)."""
    n = KINDS[kind][0]
    mid = 1.1 if n == 16 else 1.2
    cams = {
        "oblique": (R.view_matrix_ypr([mid, 0.1, 0], 1.5, 40, -55), 0.1, 10.0, 40),
        # the reference's: snake.py:322-325 (the [U] default camera's fov 60, near 0.01, far 100)
        "reference": (R.view_matrix_ypr([1.28, 0, 0], 1.5, -30, -90), 0.01, 100.0, 60),
        # ground level, 0.3 m from the chain
        "ground": (R.look_at([mid, -0.3, 0.08], [mid - 0.2, 0.0, 0.03], [0, 0, 1]), 0.02, 1.2, 60),
        # the near plane cuts through the chain, the far plane lies in front of part of the ground
        "cut": (R.view_matrix_ypr([mid, 0, 0], 1.0, 60, -25), 1.03, 1.8, 60),
    }
    out = {}
    for k, (V, near, far, fov) in cams.items():
        P = R.projection_fov(fov, aspect, near, far)
        out[k] = (V.astype(np.float32), P.astype(np.float32), near, far)
    return out


# call -> (size, shadow, env ids or None (0 .. N_ENVS - 1), camera names: one = shared)
CALLS = {
    "A": ("full", True, [3, 1, 1, 0], ["oblique", "reference", "ground", "cut"]),
    "B": ("odd", False, None, ["oblique"]),
    "C": ("odd", True, [1, 0], ["ground", "cut"]),
    "D": ("full", False, [2, 4, 0], ["reference", "oblique", "cut"]),
}
CASES = [(k, c) for k in KINDS for c in CALLS]


def call_inputs(kind, call):
    """(width, height, shadow, env_ids list, cams [n_images or 1, 32] float32, shared, per-image (near, far))."""
    size, shadow, ids, names = CALLS[call]
    W, H = SIZES[size]
    cm = cameras(kind, W / H)
    ids_l = list(range(N_ENVS)) if ids is None else ids
    shared = len(names) == 1
    arr = np.stack([np.concatenate(cm[nm][:2]) for nm in names]).astype(np.float32)
    nf = [cm[names[0] if shared else names[k]][2:] for k in range(len(ids_l))]
    return W, H, shadow, ids_l, arr, shared, nf


@functools.lru_cache(maxsize=None)
def expected(kind, call):
    """Per image of the call: (float64 model's image, float32 twin's image, retention mask at np_render.DELTA)."""
    n = KINDS[kind][0]
    W, H, shadow, ids, cams, shared, _ = call_inputs(kind, call)
    S, B = states(kind), boxes(kind)
    out = []
    for k, e in enumerate(ids):
        sc = R.scene(n, S[e].astype(np.float64), B[e])
        cam = cams[0 if shared else k].astype(np.float64)
        m64 = R.render(sc, cam[:16], cam[16:], W, H, shadow)
        sc32 = R.scene(n, S[e], B[e], dtype=np.float32)           # (the twin's forward kinematics is float32 too)
        m32 = R.render(sc32, cam[:16], cam[16:], W, H, shadow, dtype=np.float32)
        keep = R.retention_mask(sc, cam[:16], cam[16:], W, H, shadow, centre=m64)
        out.append((m64, m32, keep))
    return out
