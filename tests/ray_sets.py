"""The ray sets of tests/test_np_rays.py (CPU) and tests/test_gpu_rays.py (GPU) on the handles and states of
tests/render_scenes.py (kinds 16s, 16f, 32; 5 envs), generated from fixed seeds, and the float64 model's / the float32 twin's
records of each, computed once per process.  Both files walk the same list, so the retention displacement (np_rays.DELTA)
determined on the CPU is the one the GPU gates use, on the same rays."""
import functools

import numpy as np

import np_rays as NR
import np_render as R
import render_scenes as RS

SETS = ("fan_base", "fan_tail", "scan", "random257", "random600", "one", "degenerate")
CASES = [(k, s) for k in RS.KINDS for s in SETS]
ONE_ROWS = 256         # "one": n_rays = 1, over 256 rows (the 5 envs in turn), each row its own ray: every percentile of
#                        the GPU gates then stands on at least 30 hits (conftest.f32_gate's own threshold for a sample)


@functools.lru_cache(maxsize=None)
def scenes(kind):
    n = RS.KINDS[kind][0]
    S, B = RS.states(kind), RS.boxes(kind)
    return [R.scene(n, S[e].astype(np.float64), B[e]) for e in range(RS.N_ENVS)]


def _fan():
    """64 rays in the parent's xy plane over 360 degrees, 3 m long, from its origin; then the same ring tilted 10 degrees
    down (towards the parent's -z)."""
    a = 2 * np.pi * np.arange(64) / 64
    tilt = np.deg2rad(10.0)
    flat = 3.0 * np.stack([np.cos(a), np.sin(a), np.zeros(64)], -1)
    down = 3.0 * np.stack([np.cos(a) * np.cos(tilt), np.sin(a) * np.cos(tilt), -np.sin(tilt) * np.ones(64)], -1)
    to = np.concatenate([flat, down])
    return np.concatenate([np.zeros_like(to), to], -1)


def _scan(kind):
    """a 16 x 16 grid of vertical rays from z = 0.5 to z = -0.1 over the bounding box of the five snakes and their blocks"""
    pts = [sc["C"] for sc in scenes(kind)]
    for sc in scenes(kind):
        if sc["box"] is not None:
            c, Rb, h = sc["box"]
            pts.append(c + (np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * h) @ Rb.T)
    pts = np.concatenate(pts)
    lo, hi = pts.min(0) - 0.05, pts.max(0) + 0.05
    # (cell centres of a grid moved off the bounding box's own symmetry by an irrational fraction of a cell)
    x = lo[0] + (hi[0] - lo[0]) * (np.arange(16) + 0.5 + 0.1 * np.sqrt(2)) / 16.5
    y = lo[1] + (hi[1] - lo[1]) * (np.arange(16) + 0.5 + 0.1 * np.sqrt(3)) / 16.5
    X, Y = np.meshgrid(x, y, indexing="ij")
    frm = np.stack([X.ravel(), Y.ravel(), np.full(256, 0.5)], -1)
    to = frm.copy()
    to[:, 2] = -0.1
    return np.concatenate([frm, to], -1)


def _random(kind, env, count, rng):
    """`count` rays from a 1.5 m sphere around the chain's middle to points within 0.1 m of random cylinders' centres and,
    one in four, of the block"""
    sc = scenes(kind)[env]
    mid = sc["C"].mean(0)
    v = rng.normal(size=(count, 3))
    frm = mid + 1.5 * v / np.linalg.norm(v, axis=-1)[:, None]
    to = sc["C"][rng.integers(0, len(sc["C"]), count)]
    if sc["box"] is not None:
        c, Rb, h = sc["box"]
        onbox = c + (rng.uniform(-1, 1, (count, 3)) * h) @ Rb.T
        to = np.where((rng.uniform(size=count) < 0.25)[:, None], onbox, to)
    w = rng.normal(size=(count, 3))
    to = to + 0.1 * rng.uniform(size=(count, 1)) ** (1 / 3) * w / np.linalg.norm(w, axis=-1)[:, None]
    return np.concatenate([frm, to], -1)


# rays of "degenerate", per env, finite ones first; DEGENERATE_NONFINITE more follow on the device path
DEGENERATE = ("inside_cylinder", "inside_box", "zero_length", "level", "in_the_ground_plane", "along_axis")
DEGENERATE_NONFINITE = 3
DEG_CYL = 9            # the cylinder "inside_cylinder" starts in and "along_axis" runs along


def _degenerate(kind, env):
    sc = scenes(kind)[env]
    c, A = sc["C"][DEG_CYL], sc["A"][DEG_CYL]
    side = np.cross(A, [0.0, 0.0, 1.0] if abs(A[2]) < 0.9 else [1.0, 0.0, 0.0])
    side /= np.linalg.norm(side)
    bc = sc["box"][0] if sc["box"] is not None else np.array([1.0, 0.6, 0.1])
    return np.array([np.concatenate([c, c + 0.5 * side]),                          # starts inside cylinder DEG_CYL, leaves through its side
                     np.concatenate([bc, bc + [0.0, 0.0, 1.0]]),                   # starts inside the box (where there is one)
                     np.concatenate([c + [0, 0, 0.3], c + [0, 0, 0.3]]),           # zero length
                     np.concatenate([c + [-1, 0.2, 0.5], c + [1, 0.2, 0.5]]),      # parallel to the ground, above everything
                     [c[0] - 1, c[1] - 1, 0.0, c[0] - 2, c[1] - 2.5, 0.0],         # lies in the ground plane itself
                     np.concatenate([c + 0.2 * A, c - 0.2 * A])])                  # along the cylinder's axis


@functools.lru_cache(maxsize=None)
def call_inputs(kind, name):
    """dict(rays float32 [rows, n_rays, 6] or [n_rays, 6] (shared), env_ids list (one per row), parent_row, flags)."""
    n = RS.KINDS[kind][0]
    envs = list(range(RS.N_ENVS))
    rng = np.random.default_rng(2000 + 10 * sorted(RS.KINDS).index(kind) + SETS.index(name))
    parent = -1
    if name.startswith("fan"):
        rays, parent = _fan(), (1 if name == "fan_base" else 3 * n + 1)
    elif name == "scan":
        rays = _scan(kind)
    elif name.startswith("random"):
        rays = np.stack([_random(kind, e, int(name[6:]), rng) for e in envs])
    elif name == "one":
        envs = [k % RS.N_ENVS for k in range(ONE_ROWS)]
        rays = np.stack([_random(kind, e, 1, rng) for e in envs])
    else:
        rays = np.stack([_degenerate(kind, e) for e in envs])
    return dict(rays=rays.astype(np.float32), env_ids=envs, parent_row=parent, flags=NR.ALL)


def rows_of(inp):
    """the rays of every row, [rows, n_rays, 6] (a shared set repeated)"""
    rays = inp["rays"]
    return np.broadcast_to(rays, (len(inp["env_ids"]),) + rays.shape) if rays.ndim == 2 else rays


def model(kind, inp, dtype=np.float64, flags=None, **kw):
    """np_rays.ray_test over the rows of a call: dict of arrays [rows, n_rays, ...].  One evaluation per distinct env."""
    n = RS.KINDS[kind][0]
    S, B = RS.states(kind), RS.boxes(kind)
    rays, ids = rows_of(inp), np.asarray(inp["env_ids"])
    out = None
    for e in sorted(set(ids.tolist())):
        rows = np.nonzero(ids == e)[0]
        st = S[e].astype(np.float64) if dtype == np.float64 else S[e]
        m = NR.ray_test(n, st, B[e], rays[rows].reshape(-1, 6), inp["parent_row"], inp["flags"] if flags is None else flags,
                        dtype=dtype, **kw)
        if out is None:
            out = {k: np.zeros((len(ids), rays.shape[1]) + v.shape[1:], v.dtype) for k, v in m.items()}
        for k, v in m.items():
            out[k][rows] = v.reshape((len(rows), rays.shape[1]) + v.shape[1:])
    return out


def retained(kind, inp, delta=None, base=None):
    """np_rays.retained over the rows of a call: bool [rows, n_rays]"""
    n = RS.KINDS[kind][0]
    S, B = RS.states(kind), RS.boxes(kind)
    rays, ids = rows_of(inp), np.asarray(inp["env_ids"])
    keep = np.zeros(rays.shape[:2], bool)
    for e in sorted(set(ids.tolist())):
        rows = np.nonzero(ids == e)[0]
        b = None if base is None else {k: v[rows].reshape((-1,) + v.shape[2:]) for k, v in base.items()}
        keep[rows] = NR.retained(n, S[e].astype(np.float64), B[e], rays[rows].reshape(-1, 6), inp["parent_row"], inp["flags"],
                                 delta=delta, base=b).reshape(len(rows), -1)
    return keep


@functools.lru_cache(maxsize=None)
def expected(kind, name):
    """(float64 model's dict, float32 twin's dict, retention mask at np_rays.DELTA) of a call, arrays [rows, n_rays, ...]"""
    inp = call_inputs(kind, name)
    m64 = model(kind, inp)
    return m64, model(kind, inp, dtype=np.float32), retained(kind, inp, base=m64)
