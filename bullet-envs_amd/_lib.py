"""ctypes binding of libsnk.so (include/snk.h).

There is NO CPU fallback: if the HIP library cannot be loaded, importing the stepper
raises.  (The CPU oracle under oracle/ is test infrastructure and is never imported here.)
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SNK_LIB selects an instrumented build of the same ABI (tools/profile_phases.py); default: libsnk.so
LIB_PATH = os.environ.get("SNK_LIB") or os.path.join(_HERE, "libsnk.so")


class SnkParams(C.Structure):
    """Mirror of `snk_params` (include/snk.h)."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("abi_version", C.c_uint32),
        ("n_modules", C.c_int32), ("inertia_from_file", C.c_int32),
        ("default_mass", C.c_double), ("collision_margin", C.c_double),
        ("hull_sides", C.c_int32), ("contact_model", C.c_int32),
        ("self_collision", C.c_int32), ("obstacle", C.c_int32),
        ("obstacle_pos", C.c_double * 3), ("obstacle_half", C.c_double * 3), ("mu_obstacle", C.c_double),
        ("obstacle_mass", C.c_double),
        ("dt", C.c_double), ("gravity_z", C.c_double),
        ("lin_damping", C.c_double), ("ang_damping", C.c_double),
        ("joint_damping", C.c_double), ("max_coord_vel", C.c_double),
        ("kp", C.c_double), ("kd", C.c_double), ("max_motor_impulse", C.c_double),
        ("joint_lo", C.c_double), ("joint_hi", C.c_double),
        ("limit_erp", C.c_double), ("limit_max_impulse", C.c_double),
        ("mu_link", C.c_double), ("aniso", C.c_double * 3),
        ("contact_erp", C.c_double), ("linear_slop", C.c_double),
        ("breaking_threshold", C.c_double), ("relative_breaking_threshold", C.c_int32), ("cone_friction", C.c_int32),
        ("n_iterations", C.c_int32), ("residual_threshold", C.c_double),
        ("warm_start", C.c_int32), ("warmstarting_factor", C.c_double), ("friction_directions", C.c_int32),
        ("scaling_factor", C.c_double), ("gait", C.c_int32),
        ("servo_tol", C.c_double), ("max_counter", C.c_int32),
        ("height_threshold", C.c_double), ("energy_dt", C.c_double),
        ("alpha", C.c_double), ("beta", C.c_double), ("gamma", C.c_double),
        ("term_angle", C.c_double), ("term_index", C.c_int32),
        ("collision_force", C.c_double), ("collision_penalty", C.c_double),
        ("done_penalty", C.c_double),
        ("contact_order", C.c_int32), ("reserved0", C.c_int32),
        ("noncontact_order", C.c_int32), ("contact_erp_rule", C.c_int32),
    ]


# every symbol include/snk.h declares: name -> (restype, argtypes)
_vp = C.c_void_p
_F = C.POINTER(C.c_float)
_U8 = C.POINTER(C.c_uint8)
_I32 = C.POINTER(C.c_int32)
_D = C.POINTER(C.c_double)
SYMBOLS = {
    "snk_default_params": (None, [C.POINTER(SnkParams)]),
    "snk_create": (C.c_int, [C.POINTER(SnkParams), C.c_int32, C.c_int32, C.POINTER(_vp)]),
    "snk_destroy": (C.c_int, [_vp]),
    "snk_num_envs": (C.c_int32, [_vp]),
    "snk_obs_dim": (C.c_int32, [_vp]),
    "snk_act_dim": (C.c_int32, [_vp]),
    "snk_state_dim": (C.c_int32, [_vp]),
    "snk_record_floats": (C.c_int32, [_vp]),
    "snk_reset": (C.c_int, [_vp, _vp, _vp, _vp]),
    "snk_step": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_int32, _vp]),
    "snk_reset_pose_floats": (C.c_int32, [_vp]),
    "snk_set_reset_pose": (C.c_int, [_vp, _U8, _F]),
    "snk_get_reset_pose": (C.c_int, [_vp, _F]),
    "snk_set_reset_pose_dev": (C.c_int, [_vp, _vp, _vp, _vp]),
    "snk_step_packed": (C.c_int, [_vp, _vp, _vp, C.c_int32, _vp, C.c_int32, _vp]),
    "snk_trace_row_floats": (C.c_int32, [_vp]),
    "snk_step_traced": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int32, C.c_int32, _vp]),
    "snk_step_traced_host": (C.c_int, [_vp, _F, _F, _F, _U8, _I32, _F, C.c_int32, C.c_int32]),
    "snk_reset_host": (C.c_int, [_vp, _U8, _F]),
    "snk_step_host": (C.c_int, [_vp, _F, _F, _F, _U8, _I32, C.c_int32]),
    "snk_substep_host": (C.c_int, [_vp, _F, C.c_int32, _I32]),
    "snk_substep": (C.c_int, [_vp, _vp, C.c_int32, _vp, _vp, _vp]),
    "snk_observe": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "snk_link_state_rows": (C.c_int32, [_vp]),
    "snk_link_states": (C.c_int, [_vp, _vp, C.c_int32, _vp, _vp]),
    "snk_link_states_host": (C.c_int, [_vp, _I32, C.c_int32, _F]),
    "snk_link_inertial_offsets": (C.c_int, [C.POINTER(SnkParams), _D]),
    "snk_contact_slots": (C.c_int32, [_vp]),
    "snk_contacts": (C.c_int, [_vp, _vp, C.c_int32, _vp, _vp, _vp, _vp]),
    "snk_contacts_host": (C.c_int, [_vp, _I32, C.c_int32, _F, _F, _I32]),
    "snk_contact_links": (C.c_int, [C.POINTER(SnkParams), _I32]),
    "snk_link_pairs": (C.c_int32, [_vp]),
    "snk_closest_slots": (C.c_int32, [_vp, C.c_int32]),
    "snk_closest_points": (C.c_int, [_vp, _vp, C.c_int32, C.c_float, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp]),
    "snk_closest_points_host": (C.c_int, [_vp, _I32, C.c_int32, C.c_float, C.c_int32, C.c_int32, _F, _F, _I32]),
    "snk_copy_envs": (C.c_int, [_vp, _vp, _vp, C.c_int32, C.c_int32, _vp]),
    "snk_copy_envs_host": (C.c_int, [_vp, _I32, _I32, C.c_int32, C.c_int32]),
    "snk_get_state": (C.c_int, [_vp, _F, _F]),
    "snk_set_state": (C.c_int, [_vp, _F, _F]),
    "snk_manifold_floats": (C.c_int32, [_vp]),
    "snk_get_manifold": (C.c_int, [_vp, _F]),
    "snk_set_manifold": (C.c_int, [_vp, _F]),
    "snk_contact_overflow": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "snk_contact_histogram_bins": (C.c_int32, []),
    "snk_contact_histogram": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.c_int32]),
    "snk_contact_histogram_enable": (C.c_int, [_vp, C.c_int32]),
    "snk_get_box": (C.c_int, [_vp, _F, _F]),
    "snk_set_box": (C.c_int, [_vp, _F, _F]),
    "snk_get_obs": (C.c_int, [_vp, _F]),
    "snk_mean_height": (C.c_int, [_vp, _F]),
    "snk_link_positions": (C.c_int, [_vp, _F]),
    "snk_joint3_reaction_fz": (C.c_int, [_vp, _F]),
    "snk_set_ground_friction": (C.c_int, [_vp, _F]),
    "snk_get_ground_friction": (C.c_int, [_vp, _F]),
    "snk_debug_set_tickets": (C.c_int, [_vp, C.c_uint32]),
    "snk_debug_raise_alarm": (C.c_int, [_vp]),
    "snk_debug_noncontact_order": (C.c_int, [C.c_int32, _I32]),
    "snk_debug_rows_layout": (C.c_int, [C.c_int32, _I32]),
    "snk_debug_rows": (C.c_int, [_vp, C.c_int32, _F]),
    "snk_debug_reach_bound": (C.c_int, [C.POINTER(SnkParams), _F]),
    "snk_selftest": (C.c_int, [C.c_int32]),
    "snk_timing_enable": (C.c_int, [_vp, C.c_int32]),
    "snk_timing_read": (C.c_int, [_vp, _D, _I32]),
    "snk_model_describe": (C.c_int, [_vp, _D, _D]),
    "snk_params_derived": (C.c_int, [C.c_void_p, _D]),
    "snk_render": (C.c_int, [_vp, _vp, C.c_int32, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp]),
    "snk_render_host": (C.c_int, [_vp, _I32, C.c_int32, _F, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _U8, _F, _I32]),
    "snk_ray_test": (C.c_int, [_vp, _vp, C.c_int32, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp]),
    "snk_ray_test_host": (C.c_int, [_vp, _I32, C.c_int32, _F, C.c_int32, C.c_int32, C.c_int32, _F]),
    "snk_dyn_dofs": (C.c_int32, [_vp]),
    "snk_dynamics": (C.c_int, [_vp, _vp, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    "snk_dynamics_host": (C.c_int, [_vp, _I32, C.c_int32, C.c_int32, _F, _F]),
    "snk_jacobians": (C.c_int, [_vp, _vp, C.c_int32, _vp, _vp, C.c_int32, _vp, _vp]),
    "snk_jacobians_host": (C.c_int, [_vp, _I32, C.c_int32, _I32, _F, C.c_int32, _F]),
    "snk_apply_impulse": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_float, _vp, _vp]),
    "snk_apply_impulse_host": (C.c_int, [_vp, _U8, _F, _I32, _F, C.c_int32, C.c_int32, C.c_float, _F]),
    "snk_view_matrix_ypr": (C.c_int, [_F, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32, _F]),
    "snk_projection_fov": (C.c_int, [C.c_float, C.c_float, C.c_float, C.c_float, _F]),
    "snk_last_error": (C.c_char_p, []),
}
RENDER_SHADOW = 1      # SNK_RENDER_SHADOW
COPY_RESET_POSE = 1    # SNK_COPY_RESET_POSE
PAIRS_BOX = 1          # SNK_PAIRS_BOX: the (cylinder, obstacle box) pairs of snk_closest_points
PAIRS_LINKS = 2        # SNK_PAIRS_LINKS: its link-link pairs
CONTACT_FLOATS = 16     # SNK_CONTACT_FLOATS, floats per contact slot of snk_contacts: [point on the body 3 | point on the ground 3 |
#                         normal 3 | distance | normal force N | impulse | cylinder (2n: the box) | j | live | 0]
LINK_STATE_FLOATS = 16  # floats per row of snk_link_states: [COM 3 | quat xyzw 4 | link origin 3 | COM velocity 3 | omega 3]
RAY_FLOATS = 6          # SNK_RAY_FLOATS, a ray of snk_ray_test: [from 3 | to 3]
HIT_FLOATS = 8          # SNK_HIT_FLOATS, its record: [fraction | position 3 | normal 3 | primitive id (-1: a miss)]
RAYS_GROUND = 1         # SNK_RAYS_GROUND / _SNAKE / _BOX: what the rays can hit
RAYS_SNAKE = 2
RAYS_BOX = 4
RAYS_SHARED = 8         # SNK_RAYS_SHARED: one set of rays [n_rays, 6] for every row
RAYS_ALL = RAYS_GROUND | RAYS_SNAKE | RAYS_BOX
BIAS_VELOCITY = 1       # SNK_BIAS_VELOCITY: the Coriolis, centrifugal and gyroscopic terms of snk_dynamics' h
BIAS_GRAVITY = 2        # SNK_BIAS_GRAVITY: minus the generalised gravity force
JAC_MAX_POINTS = 256    # SNK_JAC_MAX_POINTS: points of one snk_jacobians call
WRENCH_FLOATS = 9           # SNK_WRENCH_FLOATS, a wrench of snk_apply_impulse: [force 3 | torque 3 | point 3]
IMPULSE_LINK_FRAME = 1      # SNK_IMPULSE_LINK_FRAME: force, torque and point in the link's COM frame (else world)
IMPULSE_DRY = 2             # SNK_IMPULSE_DRY: the delta only, nothing of the state written
IMPULSE_MAX_POINTS = 256    # SNK_IMPULSE_MAX_POINTS: points of one snk_apply_impulse call

#: the camera behind render() / getCameraImage when the caller gives no matrices [U]: the reference calls
#: resetDebugVisualizerCamera(1.5, -30, -90, [1.28, 0, 0]) right before its getCameraImage (snake.py:322-327) -- the reading
#: that shows what its author meant; PyBullet's own headless default cannot be known here.  fov 60, near 0.01, far 100.
DEFAULT_CAMERA = dict(distance=1.5, yaw=-30.0, pitch=-90.0, target=(1.28, 0.0, 0.0), fov=60.0, near=0.01, far=100.0)


def default_camera(width, height, distance=None, yaw=None, pitch=None, target=None):
    """(view16, proj16) of the [U] default camera for a width x height image; the four arguments override what the last
    resetDebugVisualizerCamera said."""
    d = DEFAULT_CAMERA
    view = view_matrix_ypr(d["target"] if target is None else target, d["distance"] if distance is None else distance,
                           d["yaw"] if yaw is None else yaw, d["pitch"] if pitch is None else pitch, 0.0, 2)
    return view, projection_fov(d["fov"], float(width) / float(height), d["near"], d["far"])

_lib = None


def load():
    """Load libsnk.so; raises RuntimeError with the reason when that is impossible."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "bullet-envs_amd: %s is missing -- build it with `python bullet-envs_amd/build.py` "
            "(hipcc, gfx950).  There is no CPU fallback." % LIB_PATH)
    # PyTorch-ROCm wheels bundle their own HIP/HSA runtime (same SONAME libamdhip64.so.7 as
    # /opt/rocm's).  Two HSA runtimes cannot share a GPU in one process, so when torch is
    # installed it is imported FIRST: libsnk.so's NEEDED entry then binds to the copy torch
    # already mapped and the process has exactly one runtime.  Without torch, /opt/rocm's is used.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:
        raise RuntimeError("bullet-envs_amd: cannot load %s: %s" % (LIB_PATH, e))
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error():
    return load().snk_last_error().decode()


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed: %s" % (what, last_error()))


def _call(name, *args):
    """One library call that reports by return code; the name is written once, so the message names this call."""
    check(getattr(load(), name)(*args), name)


class _ArgError(ValueError, AssertionError):
    """A caller's array or tensor does not fit the call.  Raised by _host here and by device_env's _arg, never by an
    `assert` statement: the checks in front of the C calls hold under `python -O`.  (Also an AssertionError: that is
    what the oldest of these checks raised.)"""


_PTR = {np.dtype(np.float32): _F, np.dtype(np.uint8): _U8, np.dtype(np.int32): _I32, np.dtype(np.float64): _D}


def _host(x, dtype, shape, what, says=None, optional=False, inplace=False, flat=False, row=False):
    """A caller's array as a host form reads it: contiguous, of `dtype`, of `shape` (None: any), or _ArgError "`what`
    must have shape .., got .." (`says` replaces the text in front of the comma).  optional: None stays None, an absent
    argument; inplace: the call writes into the caller's own array, so nothing is converted: it is a contiguous ndarray
    of `dtype` already; flat: any shape of that many elements, read as one row; row: one row shape[1:] stands for every
    row."""
    if x is None and optional:
        return None
    if inplace and not (isinstance(x, np.ndarray) and x.dtype == dtype and x.flags.c_contiguous):
        raise _ArgError("%s must be a C-contiguous %s ndarray" % (what, np.dtype(dtype).name))
    a = np.ascontiguousarray(x, dtype=dtype)
    if flat:
        a = a.reshape(-1)
    if row and a.shape == tuple(shape[1:]):
        a = np.ascontiguousarray(np.broadcast_to(a, shape))
    if shape is not None and a.shape != tuple(shape):
        raise _ArgError("%s, got %s" % (says or "%s must have shape %s" % (what, tuple(shape)), a.shape))
    return a


def _ptr(a):
    """The pointer of a host array as SYMBOLS types it; None, an absent argument, is NULL."""
    return None if a is None else a.ctypes.data_as(_PTR[a.dtype])


def default_params(**over):
    p = SnkParams()
    load().snk_default_params(C.byref(p))
    for k, v in over.items():
        if k in ("aniso", "obstacle_pos", "obstacle_half"):
            for i in range(3):
                getattr(p, k)[i] = v[i]
        else:
            if not hasattr(p, k):
                raise AttributeError("snk_params has no field %r" % k)
            setattr(p, k, v)
    return p


def noncontact_order(n_modules):
    """The sweep order the kernels are compiled with for snk_params::noncontact_order 1 (snk_debug_noncontact_order):
    2n entries, 0..n-1 = limit j, n..2n-1 = motor j - n, in the order of the forward sweep."""
    out = np.zeros(2 * int(n_modules), np.int32)
    _call("snk_debug_noncontact_order", int(n_modules), _ptr(out))
    return out


#: the names of snk_debug_rows_layout's 14 numbers, in its order
ROWS_LAYOUT = ("ND", "NC", "NCT", "kRows", "kFric", "kRS", "kMO", "kSpec", "kGeo", "kGeoOff", "kMmOff", "kYOff", "kRowFloats",
               "kBoxBody")


def rows_layout(n_modules):
    """The layout of the streamed-row solve's block of rows (snk_debug_rows_layout; snk_lds.hpp: Lds<N, false>) as a dict
    of ROWS_LAYOUT's names.  Host arithmetic only: no handle, no device."""
    out = np.zeros(len(ROWS_LAYOUT), np.int32)
    _call("snk_debug_rows_layout", int(n_modules), _ptr(out))
    return dict(zip(ROWS_LAYOUT, (int(x) for x in out)))


def reach_bound(params=None, **over):
    """What the kernels' bound on one substep's change of the mean height is made of (snk_debug_reach_bound):
    (longest joint-to-joint offset [m], |COM of the base link| [m], both rounded up by 1.001; fixed slack [m])."""
    p = params if params is not None else default_params(**over)
    out = np.zeros(3, np.float32)
    _call("snk_debug_reach_bound", C.byref(p), _ptr(out))
    return float(out[0]), float(out[1]), float(out[2])


def fptr(a):
    return a.ctypes.data_as(_F)


def link_inertial_offsets(n_modules=16, **params):
    """snk_link_inertial_offsets: [3n + 2, 3] float64, every link's COM in its own link frame (PyBullet's
    localInertialFramePosition; row r = Bullet link r - 1).  Host arithmetic only: no handle, no device."""
    p = default_params(n_modules=int(n_modules), **params)
    out = np.zeros((3 * int(n_modules) + 2, 3), np.float64)
    _call("snk_link_inertial_offsets", C.byref(p), _ptr(out))
    return out


def contact_links(n_modules=16, **params):
    """snk_contact_links: [2n] int32, the Bullet link index of every collision cylinder's link (PyBullet's linkIndexA of a
    contact of that cylinder; row link + 1 of link_states).  Host arithmetic only: no handle, no device."""
    return _contact_links(default_params(n_modules=int(n_modules), **params))


def _contact_links(p):
    out = np.zeros(2 * p.n_modules, np.int32)
    _call("snk_contact_links", C.byref(p), _ptr(out))
    return out


def view_matrix_ypr(target, distance, yaw, pitch, roll=0.0, up_axis=2):
    """snk_view_matrix_ypr: PyBullet's computeViewMatrixFromYawPitchRoll [U], a column-major float32 16-vector."""
    t = _host(target, np.float32, (3,), "target", "camera target must hold 3 values")
    out = np.zeros(16, np.float32)
    _call("snk_view_matrix_ypr", _ptr(t), float(distance), float(yaw), float(pitch), float(roll), int(up_axis), _ptr(out))
    return out


def projection_fov(fov, aspect, near, far):
    """snk_projection_fov: PyBullet's computeProjectionMatrixFOV [U], a column-major float32 16-vector (far == near gives
    the infinite entries the formula gives; nothing raises)."""
    out = np.zeros(16, np.float32)
    _call("snk_projection_fov", float(fov), float(aspect), float(near), float(far), _ptr(out))
    return out


def camera_block(view, proj, n_images):
    """([k, 32] float32 camera array, shared flag) from view / proj given as one 16-vector each (shared by every image)
    or as [n_images, 16] each."""
    v = np.asarray(view, dtype=np.float32).reshape(-1, 16)
    p = np.asarray(proj, dtype=np.float32).reshape(-1, 16)
    if v.shape[0] != p.shape[0] or v.shape[0] not in (1, n_images):
        raise ValueError("view / proj must be one 16-vector each or [%d, 16] each, got %s / %s"
                         % (n_images, np.shape(view), np.shape(proj)))
    return np.ascontiguousarray(np.concatenate([v, p], axis=1)), v.shape[0] == 1


def trace_row_floats(n_modules):
    """Floats per row of the step kernels' trace buffer (snk_trace_row_floats): the payload [obs 3n + 8 | link positions
    3(n + 1)] rounded up to whole 128-byte lines."""
    n = int(n_modules)
    return (3 * n + 8 + 3 * (n + 1) + 31) // 32 * 32


def trace_to_lists(trace, sub, n_modules):
    """What test mode's info holds (SnakeGymEnv.py:43-44, snake.py:292-293), from a trace of snk_step_traced: per env
    the lists (internal_observations, link_positions) of its first sub[i] rows, float64 arrays of 3n + 8 and 3(n + 1)
    values ([x.., y.., z..] of links 0, 3, ..., 3n).  Rows at and beyond sub[i] are never looked at (the kernel never
    writes them).  Pure numpy."""
    n = int(n_modules)
    no, nl = 3 * n + 8, 3 * (n + 1)
    trace = np.asarray(trace)
    sub = np.asarray(sub)
    if trace.ndim != 3 or trace.shape[0] != len(sub) or trace.shape[2] < no + nl:
        raise ValueError("trace must be [n_envs, rows, >= %d], got %s for %d envs" % (no + nl, trace.shape, len(sub)))
    if len(sub) and int(sub.max()) > trace.shape[1]:
        raise ValueError("trace holds %d rows per env, an env ran %d substeps" % (trace.shape[1], int(sub.max())))
    io, lp = [], []
    for i in range(len(sub)):
        rows = trace[i, :int(sub[i])].astype(np.float64)
        io.append([rows[s, :no].copy() for s in range(len(rows))])
        lp.append([rows[s, no:no + nl].copy() for s in range(len(rows))])
    return io, lp


class Snapshot:
    """THE definition of the simulator state of a handle's environments: what Stepper.snapshot reads, Stepper.restore
    writes, a checkpoint stores and a test-mode replay starts from.  A plain value: numpy arrays, axis 0 = environment.
    A field that is None is absent: `manifold` on a contact_model 0 handle, the box without obstacle 2, `reset_pose`
    when not asked for.  A new per-environment table is added HERE (FIELDS, Stepper.snapshot, Stepper.restore) and
    nowhere else."""
    FIELDS = ("state", "aux", "ground_friction", "manifold", "box_state", "box_manifold", "reset_pose")

    def __init__(self, state=None, aux=None, ground_friction=None, manifold=None, box_state=None, box_manifold=None,
                 reset_pose=None):
        self.state, self.aux, self.ground_friction, self.manifold = state, aux, ground_friction, manifold
        self.box_state, self.box_manifold, self.reset_pose = box_state, box_manifold, reset_pose

    @property
    def n_envs(self):
        return len(next(v for v in map(self.__dict__.get, self.FIELDS) if v is not None))

    def __getitem__(self, idx):
        """numpy indexing on axis 0 of every field present: snap[perm], a subset, replicas (src[idx] = e; snap[src])."""
        return Snapshot(**{k: None if v is None else v[idx] for k, v in self.__dict__.items()})

    def arrays(self):
        """The fields as a checkpoint stores them: an empty float32 array stands for an absent one."""
        return {k: np.zeros(0, np.float32) if self.__dict__[k] is None else self.__dict__[k] for k in self.FIELDS}

    @classmethod
    def from_arrays(cls, mapping):
        """The inverse of arrays(); a key the mapping does not have is an absent field too."""
        return cls(**{k: mapping[k] for k in cls.FIELDS if k in mapping and np.size(mapping[k])})


class Stepper:
    """Thin owner of one `snk_handle`: N environments on one GPU (host-buffer API)."""

    def __init__(self, n_envs, device=0, params=None, **over):
        self.lib = load()
        self.params = params if params is not None else default_params(**over)
        h = _vp()
        _call("snk_create", C.byref(self.params), int(n_envs), int(device), C.byref(h))
        self.h = h
        self.n_envs = int(n_envs)
        self.device = int(device)
        self.n = self.params.n_modules
        self.obs_dim = self.lib.snk_obs_dim(h)
        self.act_dim = self.lib.snk_act_dim(h)
        self.state_dim = self.lib.snk_state_dim(h)

    def close(self):
        if getattr(self, "h", None):
            self.lib.snk_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, name, *args):
        """Every call on the handle that reports by return code: the name is written once."""
        check(getattr(self.lib, name)(self.h, *args), name)

    def _count(self, name, *args):
        """The getters whose zero is a refusal: the count, or the library's reason."""
        k = int(getattr(self.lib, name)(self.h, *args))
        if k == 0:
            raise RuntimeError("%s failed: %s" % (name, last_error()))
        return k

    def _zeros(self, *shape, dtype=np.float32):
        """a fresh per-env table [n_envs, *shape]"""
        return np.zeros((self.n_envs,) + shape, dtype=dtype)

    def _read(self, name, *shape):
        """The getters of one float32 table [n_envs, *shape]."""
        out = self._zeros(*shape)
        self._call(name, _ptr(out))
        return out

    # ---- host-buffer calls ----
    def reset(self, mask=None):
        obs = self._zeros(self.obs_dim)
        self._call("snk_reset_host", _ptr(_host(mask, np.uint8, (self.n_envs,), "mask", optional=True)), _ptr(obs))
        return obs

    def _step(self, actions, vec_mode, traced):
        """step and step_traced, as step_host is in C: the trace is the only variation."""
        _host(actions, np.float32, (self.n_envs, self.act_dim), "actions", inplace=True)
        obs = np.empty((self.n_envs, self.obs_dim), dtype=np.float32)
        rew = np.empty(self.n_envs, dtype=np.float32)
        done = np.empty(self.n_envs, dtype=np.uint8)
        sub = np.empty(self.n_envs, dtype=np.int32)
        out = (_ptr(actions), _ptr(obs), _ptr(rew), _ptr(done), _ptr(sub))
        if not traced:
            self._call("snk_step_host", *out, 1 if vec_mode else 0)
            return obs, rew, done.astype(bool), sub
        trace = np.full(self.trace_shape(), np.nan, dtype=np.float32)
        self._call("snk_step_traced_host", *out, _ptr(trace), trace.shape[1], 1 if vec_mode else 0)
        return obs, rew, done.astype(bool), sub, trace

    def step(self, actions, vec_mode=True):
        """actions float32 [n_envs, act_dim], clipped in place.  Returns obs, rew, done, substeps."""
        return self._step(actions, vec_mode, False)

    def trace_shape(self):
        """[n_envs, rows, floats per row] of the trace step_traced returns (rows = max_counter + 1)."""
        return (self.n_envs, int(self.params.max_counter) + 1, int(self.lib.snk_trace_row_floats(self.h)))

    def step_traced(self, actions, vec_mode=True):
        """step() that also records every physics substep (snk_step_traced_host).  Returns obs, rew, done, substeps,
        trace; trace [n_envs, max_counter + 1, row] float32: row s < substeps[i] of env i = [observation after substep s
        (3n + 8) | link positions (3(n + 1), x.. y.. z..) | padding]; the other rows are left as allocated (NaN here)."""
        return self._step(actions, vec_mode, True)

    def substep(self, targets, k=1):
        info = self._zeros(2, dtype=np.int32)
        self._call("snk_substep_host", _ptr(_host(targets, np.float32, (self.n_envs, self.n), "targets")), int(k), _ptr(info))
        return info

    def debug_rows_layout(self):
        """rows_layout of this handle's chain length."""
        return rows_layout(self.n)

    def debug_rows(self):
        """[n_envs, kRowFloats] float32: every env's block of streamed rows as its last substep left it (snk_debug_rows:
        streamed-row handles of at most as many envs as resident waves, right after substep())."""
        out = self._zeros(self.debug_rows_layout()["kRowFloats"])
        for e in range(self.n_envs):
            self._call("snk_debug_rows", e, _ptr(out[e]))
        return out

    def _table(self, x, what, *shape):
        """the pointer of a caller's float32 table [n_envs, *shape] (None, where the call allows it: NULL)"""
        return _ptr(_host(x, np.float32, (self.n_envs,) + shape, what, optional=True))

    def get_state(self):
        s, a = self._zeros(self.state_dim), self._zeros(self.n + 2)
        self._call("snk_get_state", _ptr(s), _ptr(a))
        return s, a

    def set_state(self, state=None, aux=None):
        self._call("snk_set_state", self._table(state, "state", self.state_dim), self._table(aux, "aux", self.n + 2))

    def get_reset_pose(self):
        """The reset-pose table (snk_get_reset_pose): [n_envs, 7 + n] = per env [position 3 | quaternion xyzw 4 | joint
        angles n], what the env's next soft reset -- reset() or the step kernel's own on `done` -- lands on."""
        return self._read("snk_get_reset_pose", 7 + self.n)

    def set_reset_pose(self, pose, mask=None):
        """snk_set_reset_pose: rows [position 3 | quaternion xyzw 4 | joint angles n] for the envs of `mask` (None: all).
        pose is [n_envs, 7 + n], or one row [7 + n] that every (masked) env gets.  Rows of unmasked envs are ignored."""
        W = 7 + self.n
        p = _host(pose, np.float32, (self.n_envs, W), "pose",
                  "reset pose must have shape (%d, %d) or (%d,)" % (self.n_envs, W, W), row=True)
        m = _host(None if mask is None else np.asarray(mask) != 0, np.uint8, (self.n_envs,), "mask", optional=True)
        self._call("snk_set_reset_pose", _ptr(m), _ptr(p))

    def set_reset_pose_device(self, pose_ptr, mask_ptr=0, stream=0):
        """snk_set_reset_pose_dev: the same update from device buffers ([n_envs, 7 + n] f32, mask [n_envs] u8 or 0 for
        all), asynchronous on `stream`; nothing is validated."""
        self._call("snk_set_reset_pose_dev", mask_ptr, pose_ptr, stream)

    def get_manifold(self):
        """contact_model 1: [n_envs, 2n, 29] contact cache (see snk.h); None for a contact_model 0 handle."""
        if self.lib.snk_manifold_floats(self.h) == 0:
            return None
        return self._read("snk_get_manifold", 2 * self.n, 29)

    def set_manifold(self, m):
        self._call("snk_set_manifold", _ptr(_host(m, np.float32, (self.n_envs, 2 * self.n, 29), "manifold")))

    def get_box(self):
        """obstacle 2: (state [n_envs, 13], manifold with the plane [n_envs, 29]) of the free box."""
        s, m = self._zeros(13), self._zeros(29)
        self._call("snk_get_box", _ptr(s), _ptr(m))
        return s, m

    def set_box(self, state=None, manifold=None):
        self._call("snk_set_box", self._table(state, "state", 13), self._table(manifold, "manifold", 29))

    def snapshot(self, reset_pose=True):
        """The simulator state of every env as a Snapshot (the EFFECTIVE friction, read back from the device);
        reset_pose=False leaves the reset-pose table out (a replay that only substeps never reads it)."""
        state, aux = self.get_state()
        box = self.get_box() if self.params.obstacle == 2 else (None, None)
        return Snapshot(state, aux, self.get_ground_friction(), self.get_manifold(), box[0], box[1],
                        self.get_reset_pose() if reset_pose else None)

    def restore(self, snap):
        """Writes every field of `snap` that is present, through the setters above, in one fixed order: friction, state
        and aux, contact cache, box, reset poses."""
        if snap.n_envs != self.n_envs:
            raise ValueError("snapshot holds %d environments, this handle %d" % (snap.n_envs, self.n_envs))
        if snap.ground_friction is not None:
            self.set_ground_friction(snap.ground_friction)
        if snap.state is not None or snap.aux is not None:
            self.set_state(snap.state, snap.aux)
        if snap.manifold is not None:
            self.set_manifold(snap.manifold)
        if snap.box_state is not None or snap.box_manifold is not None:
            self.set_box(snap.box_state, snap.box_manifold)
        if snap.reset_pose is not None:
            self.set_reset_pose(snap.reset_pose)

    def contact_overflow(self):
        """snk_contact_overflow since the handle was created: (substeps with more contact points than the solve's slots
        -- on a register-resident 16-link handle those are solved by the streamed-row solve with every point, so this is
        a count of slower substeps --, points left without rows (structurally zero: the streamed-row solve has a slot for
        every point the manifolds can hold), link-link / obstacle contacts left out).  The last two at zero mean Bullet's
        'no limit' held."""
        out = (C.c_uint64 * 3)()
        self._call("snk_contact_overflow", out)
        return int(out[0]), int(out[1]), int(out[2])

    def contact_histogram_enable(self, on=True):
        """Switches the per-substep counting on or off (off after creation: one atomic per substep, 0.7 % of the rate)."""
        self._call("snk_contact_histogram_enable", 1 if on else 0)

    def contact_histogram(self, reset=False):
        """snk_contact_histogram: out[k] = physics substeps that ran with k contact points while the counting was enabled
        (since the last call with reset=True); the last bin collects everything beyond it."""
        n = int(self.lib.snk_contact_histogram_bins())
        out = (C.c_uint64 * n)()
        self._call("snk_contact_histogram", out, 1 if reset else 0)
        return np.array(out[:], dtype=np.uint64)

    def get_obs(self):
        return self._read("snk_get_obs", self.obs_dim)

    def mean_height(self):
        return self._read("snk_mean_height")

    def link_positions(self):
        """[n_envs, 3(n+1)]: getLinkPositions of every env ([x.., y.., z..] of links 0,3,...,3n)."""
        return self._read("snk_link_positions", 3 * (self.n + 1))

    def joint3_reaction_fz(self):
        """Fz of the first motor joint's reaction (Bullet joint 3) after the last substep, [n_envs]."""
        return self._read("snk_joint3_reaction_fz")

    def set_ground_friction(self, mu):
        self._call("snk_set_ground_friction", _ptr(_host(mu, np.float32, (self.n_envs,), "mu")))

    def get_ground_friction(self):
        """The effective per-env plane friction (ones unless set), read back from the device."""
        return self._read("snk_get_ground_friction")

    def debug_set_tickets(self, base):
        self._call("snk_debug_set_tickets", int(base) & 0xFFFFFFFF)

    def debug_raise_alarm(self):
        """Test hook: the scheduler's alarm raised from the host (include/snk.h); the handle is poisoned afterwards."""
        self._call("snk_debug_raise_alarm")

    def model_describe(self):
        bodies = np.zeros((self.n + 1, 10))
        origins = np.zeros((self.n + 1, 3))
        self._call("snk_model_describe", _ptr(bodies), _ptr(origins))
        return bodies, origins

    # ---- device-pointer calls (torch tensors own the memory; a pointer 0 is NULL: ctypes converts it) ----
    def step_device(self, actions_ptr, obs_ptr, rew_ptr, done_ptr, sub_ptr=0, vec_mode=True, stream=0):
        self._call("snk_step", actions_ptr, obs_ptr, rew_ptr, done_ptr, sub_ptr, 1 if vec_mode else 0, stream)

    def step_traced_device(self, actions_ptr, obs_ptr, rew_ptr, done_ptr, sub_ptr, trace_ptr, trace_rows, vec_mode=True,
                           stream=0):
        """snk_step_traced: snk_step plus one trace row per physics substep, [n_envs x trace_rows x trace row floats] f32
        at trace_ptr (128-byte aligned); sub_ptr is required (it says how many rows of each env are valid)."""
        self._call("snk_step_traced", actions_ptr, obs_ptr, rew_ptr, done_ptr, sub_ptr, trace_ptr, int(trace_rows),
                   1 if vec_mode else 0, stream)

    def step_packed_device(self, actions_ptr, packed_ptr, row_stride, sub_ptr=0, vec_mode=True, stream=0):
        """snk_step_packed: rows [obs | reward f32 | done u32] of `row_stride` floats in one device buffer."""
        self._call("snk_step_packed", actions_ptr, packed_ptr, int(row_stride), sub_ptr, 1 if vec_mode else 0, stream)

    def reset_device(self, mask_ptr=0, obs_ptr=0, stream=0):
        self._call("snk_reset", mask_ptr, obs_ptr, stream)

    # ---- the tensor seam: substeps, read-outs, link states and forks on device pointers (0: none) ----
    def substep_device(self, targets_ptr, k=1, active_ptr=0, info_ptr=0, stream=0):
        """snk_substep: k physics substeps towards targets [n_envs, n] f32 for the envs whose byte of active [n_envs] u8
        is non-zero (0: all); info [n_envs, 2] i32.  Asynchronous on `stream`."""
        self._call("snk_substep", targets_ptr, int(k), active_ptr, info_ptr, stream)

    def observe_device(self, obs_ptr=0, height_ptr=0, linkpos_ptr=0, stream=0):
        """snk_observe: observation [n_envs, obs_dim], mean height [n_envs], link positions [n_envs, 3(n+1)], each f32
        or 0.  Asynchronous on `stream`."""
        self._call("snk_observe", obs_ptr, height_ptr, linkpos_ptr, stream)

    @property
    def link_rows(self):
        """3n + 2: rows per env of link_states (row r = Bullet link r - 1)."""
        return int(self.lib.snk_link_state_rows(self.h))

    def link_states_device(self, ids_ptr, n_rows, out_ptr, stream=0):
        """snk_link_states: out [n_rows, 3n + 2, 16] f32 for the envs ids [n_rows] i32 (0: envs 0 .. n_rows - 1)."""
        self._call("snk_link_states", ids_ptr, int(n_rows), out_ptr, stream)

    def copy_envs_device(self, src_ptr, dst_ptr, n_pairs, reset_pose=False, stream=0):
        """snk_copy_envs: env dst[i] becomes env src[i] (ids [n_pairs] i32 on the device; nothing validated)."""
        self._call("snk_copy_envs", src_ptr, dst_ptr, int(n_pairs), COPY_RESET_POSE if reset_pose else 0, stream)

    def _ids(self, env_ids):
        """(the pointer of an `env_ids` argument as an int32 list, NULL for None: all envs; how many envs it names)"""
        ids = _host(env_ids, np.int32, None, "env_ids", optional=True, flat=True)
        return _ptr(ids), self.n_envs if ids is None else len(ids)

    def link_states(self, env_ids=None):
        """snk_link_states_host: [k, 3n + 2, 16] float32 of the envs `env_ids` (None: all; ids may repeat, any order):
        per link [COM 3 | quaternion xyzw 4 | link-frame origin 3 | COM velocity 3 | angular velocity 3], world frame."""
        idp, k = self._ids(env_ids)
        out = np.zeros((max(k, 1), 3 * self.n + 2, LINK_STATE_FLOATS), np.float32)
        self._call("snk_link_states_host", idp, k, _ptr(out))
        return out

    @property
    def contact_slots(self):
        """snk_contact_slots: contact slots per env, 8n (+ 4 with the free box); raises on a contact_model 0 handle."""
        return self._count("snk_contact_slots")

    def contacts_device(self, ids_ptr, n_rows, points_ptr=0, force_ptr=0, count_ptr=0, stream=0):
        """snk_contacts: points [n_rows, slots, 16] f32, force [n_rows, 2n + 1] f32, count [n_rows] i32 (each a device
        pointer or 0) for the envs ids [n_rows] i32 (0: envs 0 .. n_rows - 1).  Asynchronous on `stream`."""
        self._call("snk_contacts", ids_ptr, int(n_rows), points_ptr, force_ptr, count_ptr, stream)

    def contacts(self, env_ids=None):
        """snk_contacts_host: (points [k, slots, 16] float32, force [k, 2n + 1] float32, count [k] int32) of the envs
        `env_ids` (None: all; ids may repeat, any order), from the contact cache at the current pose.  A slot (4 c + j:
        cached point j of cylinder c; the last four of an obstacle 2 handle: the free box) is [point on the body 3 | point
        on the ground 3 | normal 3 | distance | normal force N | impulse | c (2n: the box) | j | live | 0], sixteen zeros
        when not live; force sums a cylinder's live slots, entry 2n the box's."""
        idp, k = self._ids(env_ids)
        slots = self.contact_slots
        points = np.zeros((max(k, 1), slots, CONTACT_FLOATS), np.float32)
        force = np.zeros((max(k, 1), 2 * self.n + 1), np.float32)
        count = np.zeros(max(k, 1), np.int32)
        self._call("snk_contacts_host", idp, k, _ptr(points), _ptr(force), _ptr(count))
        return points, force, count

    def contact_links(self):
        """snk_contact_links of this handle's parameters (module function contact_links)."""
        return _contact_links(self.params)

    @property
    def link_pairs(self):
        """snk_link_pairs: the link-link pairs of the chain, C(2n, 2) - (2n - 1) (465 / 1953)."""
        return self._count("snk_link_pairs")

    def closest_slots(self, max_pairs):
        """snk_closest_slots: slots per env of closest_points' table, 2n + max_pairs."""
        return self._count("snk_closest_slots", int(max_pairs))

    def closest_points_device(self, ids_ptr, n_rows, distance, flags, max_pairs, points_ptr=0, clearance_ptr=0, count_ptr=0,
                              stream=0):
        """snk_closest_points: points [n_rows, 2n + max_pairs, 16] f32, clearance [n_rows, 2, 2n] f32, count [n_rows, 2] i32
        (each a device pointer or 0) for the envs ids [n_rows] i32 (0: envs 0 .. n_rows - 1).  Asynchronous on `stream`."""
        self._call("snk_closest_points", ids_ptr, int(n_rows), float(distance), int(flags), int(max_pairs), points_ptr,
                   clearance_ptr, count_ptr, stream)

    def closest_points(self, distance, env_ids=None, flags=PAIRS_BOX | PAIRS_LINKS, max_pairs=None):
        """snk_closest_points_host: (points [k, 2n + max_pairs, 16] float32, clearance [k, 2, 2n] float32, count [k, 2]
        int32) of the envs `env_ids` (None: all; ids may repeat, any order) at the current pose: the link-box and link-link
        pairs closer than `distance` (snk.h, "The closest points").  Slot c < 2n is the pair (cylinder c, box); the found
        link-link pairs follow, compact, in the solver's order, the first `max_pairs` of them (None: room for every
        pair).  A record is [point on cylinder a 3 | point on B 3 | normal on B 3 | distance | tier | 0 | a | b (2n: the
        box) | live | 0]; clearance is min(found distances, distance) per cylinder for the box (row 0) and the other links
        (row 1); count = (box pairs, link-link pairs) found, the latter not clipped to max_pairs."""
        idp, k = self._ids(env_ids)
        mp = self.link_pairs if max_pairs is None else int(max_pairs)
        ok = 0 <= mp <= 4096                                      # (the library refuses the rest by name; no huge buffers first)
        points = np.zeros((max(k, 1), 2 * self.n + (mp if ok else 0), CONTACT_FLOATS), np.float32)
        clearance = np.zeros((max(k, 1), 2, 2 * self.n), np.float32)
        count = np.zeros((max(k, 1), 2), np.int32)
        self._call("snk_closest_points_host", idp, k, float(distance), int(flags), mp, _ptr(points), _ptr(clearance),
                   _ptr(count))
        return points, clearance, count

    def copy_envs(self, src, dst, reset_pose=False):
        """snk_copy_envs_host: env dst[i] becomes env src[i] in everything a Snapshot holds (the reset pose only with
        reset_pose=True).  Refused with the index, nothing written: an id outside the handle, a repeated dst, a dst
        that is also a src."""
        s = _host(src, np.int32, None, "src", flat=True)
        d = _host(dst, np.int32, None, "dst", flat=True)
        if len(s) != len(d):
            raise ValueError("src and dst must name as many envs each, got %d and %d" % (len(s), len(d)))
        self._call("snk_copy_envs_host", _ptr(s), _ptr(d), len(s), COPY_RESET_POSE if reset_pose else 0)

    @staticmethod
    def link_inertial_offsets(n_modules=16, **params):
        """snk_link_inertial_offsets (module function link_inertial_offsets)."""
        return link_inertial_offsets(n_modules, **params)

    # ---- the ray caster (snk_render / snk_render_host) ----
    def render(self, view, proj, width, height, env_ids=None, shadow=False, depth=True, seg=True):
        """snk_render_host: images of the envs `env_ids` (None: all; ids may repeat, any order) from their current state.
        view / proj: column-major 16-vectors, one pair shared by every image or [n_images, 16] each.  Returns
        (rgba [k, height, width, 4] uint8, depth [k, height, width] float32 or None, seg int32 primitive ids or None)."""
        idp, k = self._ids(env_ids)
        cams, shared = camera_block(view, proj, k)
        W, H = int(width), int(height)
        ok = 1 <= W <= 4096 and 1 <= H <= 4096 and k >= 1        # (the library refuses the rest by name; no huge buffers first)
        rgba = np.zeros((k, H, W, 4) if ok else (1,), np.uint8)
        dep = np.zeros((k, H, W), np.float32) if depth and ok else None
        sg = np.zeros((k, H, W), np.int32) if seg and ok else None
        self._call("snk_render_host", idp, k, _ptr(cams), 1 if shared else 0, W, H, RENDER_SHADOW if shadow else 0,
                   _ptr(rgba), _ptr(dep), _ptr(sg))
        return rgba, dep, sg

    def render_device(self, ids_ptr, n_images, cams_ptr, shared, width, height, flags, rgba_ptr, depth_ptr=0, seg_ptr=0,
                      stream=0):
        """snk_render: every buffer a device pointer (0: none), asynchronous on `stream`."""
        self._call("snk_render", ids_ptr, int(n_images), cams_ptr, 1 if shared else 0, int(width), int(height), int(flags),
                   rgba_ptr, depth_ptr, seg_ptr, stream)

    # ---- the ray test (snk_ray_test / snk_ray_test_host) ----
    def ray_test(self, rays, env_ids=None, parent_row=-1, flags=RAYS_ALL):
        """snk_ray_test_host: hit records [k, n_rays, 8] float32 of the envs `env_ids` (None: all; ids may repeat, any
        order) at the current pose.  rays: [k, n_rays, 6] float32, [from 3 | to 3] per ray, or [n_rays, 6]: one set shared by
        every row.  parent_row -1: world coordinates; r: the frame of row r of link_states of the row's own env (origin the
        link's COM; PyBullet's parentLinkIndex L is row L + 1).  flags: RAYS_GROUND | RAYS_SNAKE | RAYS_BOX, what can be
        hit.  A record is [hit fraction | position 3 | outward normal 3 | primitive id: 0 ground, 1 + c cylinder c, 1 + 2n
        the box], world frame; a miss is [1, 0, 0, 0, 0, 0, 0, -1] (snk.h, "The ray test")."""
        idp, k = self._ids(env_ids)
        rays = _host(rays, np.float32, None, "rays")
        if rays.ndim not in (2, 3) or rays.shape[-1] != RAY_FLOATS or (rays.ndim == 3 and rays.shape[0] != k):
            raise ValueError("rays must be [%d, n_rays, 6] or [n_rays, 6], got %s" % (k, rays.shape))
        shared = rays.ndim == 2
        R = int(rays.shape[-2])
        ok = k >= 1 and 1 <= R <= 65536 and k * R <= 1 << 28      # (the library refuses the rest by name; no huge buffers first)
        hits = np.zeros((k, R, HIT_FLOATS) if ok else (1,), np.float32)
        self._call("snk_ray_test_host", idp, k, _ptr(rays if rays.size else None), R, int(parent_row),
                   (int(flags) & ~RAYS_SHARED) | (RAYS_SHARED if shared else 0), _ptr(hits))
        return hits

    def ray_test_device(self, ids_ptr, n_rows, rays_ptr, n_rays, parent_row, flags, hits_ptr, stream=0):
        """snk_ray_test: every buffer a device pointer (ids 0: envs 0 .. n_rows - 1), asynchronous on `stream`."""
        self._call("snk_ray_test", ids_ptr, int(n_rows), rays_ptr, int(n_rays), int(parent_row), int(flags), hits_ptr, stream)

    # ---- the dynamics queries (snk_dynamics / snk_jacobians and their host forms) ----
    @property
    def dyn_dofs(self):
        """snk_dyn_dofs: nd = 6 + n, the components of u = [omega 3 | v of the root origin 3 | qd n]."""
        return self._count("snk_dyn_dofs")

    def dynamics_device(self, ids_ptr, n_rows, flags, mass_ptr=0, bias_ptr=0, stream=0):
        """snk_dynamics: mass [n_rows, nd, nd] f32, bias [n_rows, nd] f32 (each a device pointer or 0) for the envs ids
        [n_rows] i32 (0: envs 0 .. n_rows - 1).  Asynchronous on `stream`."""
        self._call("snk_dynamics", ids_ptr, int(n_rows), int(flags), mass_ptr, bias_ptr, stream)

    def dynamics(self, env_ids=None, flags=BIAS_VELOCITY | BIAS_GRAVITY, mass=True, bias=True):
        """snk_dynamics_host: (M [k, nd, nd] float32 or None, h [k, nd] float32 or None) of the envs `env_ids` (None: all;
        ids may repeat, any order) at the state they hold: M du/dt + h = Q over u = [omega 3 | v of the root origin 3 | qd
        n].  flags: BIAS_VELOCITY | BIAS_GRAVITY, the terms of h (snk.h, "The dynamics queries")."""
        idp, k = self._ids(env_ids)
        nd = self.n + 6
        M = np.zeros((max(k, 1), nd, nd), np.float32) if mass else None
        h = np.zeros((max(k, 1), nd), np.float32) if bias else None
        self._call("snk_dynamics_host", idp, k, int(flags), _ptr(M), _ptr(h))
        return M, h

    def jacobians_device(self, ids_ptr, n_rows, link_rows_ptr, local_ptr, n_points, jac_ptr, stream=0):
        """snk_jacobians: jac [n_rows, n_points, 6, nd] f32 for the links link_rows [n_points] i32 (rows of link_states) and
        the points local [n_points, 3] f32 in their COM frames (0: the COMs); every buffer a device pointer.  Asynchronous on
        `stream`."""
        self._call("snk_jacobians", ids_ptr, int(n_rows), link_rows_ptr, local_ptr, int(n_points), jac_ptr, stream)

    def jacobians(self, link_rows, local=None, env_ids=None):
        """snk_jacobians_host: [k, n_points, 6, nd] float32 of the envs `env_ids` (None: all; ids may repeat, any order):
        per point rows 0-2 the world linear velocity per unit of each component of u, rows 3-5 the link's angular velocity.
        link_rows: rows of link_states (Bullet link + 1), one list for every env; local: [n_points, 3] points in the links'
        COM frames (None: the COMs)."""
        idp, k = self._ids(env_ids)
        rows = _host(link_rows, np.int32, None, "link_rows", flat=True)
        P = len(rows)
        loc = _host(local, np.float32, (P, 3), "local", "local must be [%d, 3]" % P, optional=True)
        ok = 1 <= P <= JAC_MAX_POINTS                         # (the library refuses the rest by name; no huge buffers first)
        jac = np.zeros((max(k, 1), P, 6, self.n + 6) if ok else (1,), np.float32)
        self._call("snk_jacobians_host", idp, k, _ptr(rows if P else None), _ptr(loc), P, _ptr(jac))
        return jac

    # ---- the applied forces (snk_apply_impulse and its host form) ----
    def apply_impulse_device(self, active_ptr=0, gen_force_ptr=0, link_rows_ptr=0, wrench_ptr=0, n_points=0, flags=0,
                             seconds=0.0, delta_ptr=0, stream=0):
        """snk_apply_impulse: u += seconds x M^-1 Q for the envs whose byte of active [n_envs] u8 is non-zero (0: all), Q =
        gen_force [n_envs, nd] f32 + the wrenches [n_envs, n_points, 9] f32 on the links link_rows [n_points] i32; delta
        [n_envs, nd] f32.  Every buffer a device pointer or 0.  Asynchronous on `stream`."""
        self._call("snk_apply_impulse", active_ptr, gen_force_ptr, link_rows_ptr, wrench_ptr, int(n_points), int(flags),
                   float(seconds), delta_ptr, stream)

    def apply_impulse(self, gen_force=None, link_rows=None, wrenches=None, flags=0, seconds=None, active=None):
        """snk_apply_impulse_host: the velocity of the active envs (active [n_envs] bool / uint8; None: all) becomes u +
        delta, delta = seconds x M^-1 Q (flags IMPULSE_DRY: nothing is written), and delta [n_envs, nd] float32 comes back.
        Q = gen_force [n_envs, nd] (moment about the root origin 3 | force 3 | joint torques n; None: none) + the wrenches
        [n_envs, P, 9] = [force 3 | torque 3 | point 3] on the links link_rows [P] (rows of link_states; one list for every
        env), in world axes at a world point, or with IMPULSE_LINK_FRAME in the link's COM frame.  seconds None: the
        handle's dt as the kernels hold it (snk.h, "The applied forces")."""
        nd = self.n + 6
        E = self.n_envs
        gf = _host(gen_force, np.float32, (E, nd), "gen_force", "gen_force must be [%d, %d]" % (E, nd), optional=True)
        rows = _host([] if link_rows is None else link_rows, np.int32, None, "link_rows", flat=True)
        P = len(rows)
        if P and wrenches is None:
            raise ValueError("link_rows without wrenches")
        wr = _host(wrenches, np.float32, (E, P, WRENCH_FLOATS), "wrenches",
                   "wrenches must be [%d, %d, %d]" % (E, P, WRENCH_FLOATS), optional=True)
        act = _host(active, np.uint8, (E,), "active", "active must be [%d]" % E, optional=True, flat=True)
        delta = self._zeros(nd)
        self._call("snk_apply_impulse_host", _ptr(act), _ptr(gf), _ptr(rows if P else None), _ptr(wr if P else None), P,
                   int(flags), float(np.float32(self.params.dt)) if seconds is None else float(seconds), _ptr(delta))
        return delta

    def timing_enable(self, capacity):
        self._call("snk_timing_enable", int(capacity))

    def timing_read(self):
        ms = C.c_double()
        cnt = C.c_int32()
        self._call("snk_timing_read", C.byref(ms), C.byref(cnt))
        return ms.value, cnt.value
