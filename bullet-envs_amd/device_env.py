"""Device-resident and multi-GPU forms of the vector env.

DeviceVecEnv   torch CUDA(=HIP) tensors in, tensors out; the step kernel is enqueued on
               torch's current stream, nothing touches the host.
DeviceWorld    the physics BELOW the fused env-step on the same terms: masked substeps, observation / mean height /
               link positions, the states of all 3n + 2 links, resets and env forks, each one launch on the current
               stream.  An env with another reward, termination rule, gait or control rate -- or a sampling-based
               controller forking states -- is torch code over these calls and never leaves the GPU.
ShardedVecEnv  one process per GPU (torch.distributed, backend "nccl" = RCCL over xGMI).
               Global env g lives on rank g // envs_per_rank for its whole life; the
               physics never communicates.  Per env-step there is exactly one exchange each
               way with the trainer rank: actions scatter (N*A*4 B per rank) and one packed
               [obs | reward | done] gather ((O+2)*4 B per env).  A gather-to-root is
               inbound-link-parallel on the fully connected xGMI mesh, so it is not
               ring-bound.

Replaces the Pipe fan-out/fan-in of SubprocVecEnv (ppo/multiprocessing_env.py:119-128).
torch is plumbing here (device memory, streams, process groups); it computes nothing.
"""
import numpy as np

from . import _lib
from .snake_env import FrozenInfo, params_from_args


class _TensorArgs(object):
    """What DeviceVecEnv and DeviceWorld share: the current stream, and a caller's tensors as the kernels take them
    (self.torch, self.device and self.num_envs are the subclass's)."""

    def _stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def _arg(self, x, what, dtypes, shape, optional=False, more=None, flat=False):
        """A caller's tensor as the kernels read it: on this device, of one of `dtypes`, of `shape`, contiguous -- THE
        check between a caller's tensor and what a kernel reads and writes, raised (_lib._ArgError), never an `assert`.
        optional: None stays None, an absent argument; more = (d, "rows"): dimension d may be larger than asked (the
        kernel is told its size); flat: any shape of as many elements."""
        t = self.torch
        if x is None and optional:
            return None
        if not isinstance(x, t.Tensor) or not x.is_cuda or x.device != self.device:
            raise _lib._ArgError("%s must be a CUDA tensor on %s" % (what, self.device))
        if x.dtype not in dtypes:
            raise _lib._ArgError("%s must be %s, got %s" % (what, " or ".join(str(d) for d in dtypes), x.dtype))
        got, want = tuple(x.shape), tuple(shape)
        if got != want:
            if flat:
                fits = x.numel() == int(np.prod(want))
            else:
                d = more[0] if more else 0
                fits = more and len(got) == len(want) and got[d] > want[d] and got[:d] + got[d + 1:] == want[:d] + want[d + 1:]
            if not fits:
                raise _lib._ArgError("%s must have shape %s%s, got %s" % (what, want, " (or more %s)" % more[1] if more else
                                                                         " (or as many elements)" if flat else "", got))
        if not x.is_contiguous():
            raise _lib._ArgError("%s must be contiguous" % what)
        return x

    def _out(self, out, what, shape, dtype=None):
        t = self.torch
        dtype = t.float32 if dtype is None else dtype
        if out is None:
            return t.empty(shape, dtype=dtype, device=self.device)
        return self._arg(out, what, (dtype,), shape)

    def _want(self, spec, shape, dtype=None):
        """_out of an output a query may leave out: spec is None (not wanted) or (its name in a message, the caller's
        tensor or None for a fresh one)"""
        return None if spec is None else self._out(spec[1], spec[0], shape, dtype)

    @staticmethod
    def _ptr(x):
        """a tensor's device pointer; 0, the kernels' NULL, for an absent one"""
        return 0 if x is None else x.data_ptr()

    def _reset_pose_dev(self, pose, mask):
        """snk_set_reset_pose_dev on the current stream: pose [E, 7 + n] float32, mask uint8 / bool [E] or None"""
        t = self.torch
        pose = self._arg(pose, "pose", (t.float32,), (self.num_envs, 7 + self.stepper.n))
        mask = self._arg(mask, "mask", (t.uint8, t.bool), (self.num_envs,), optional=True)   # (a bool is one byte, 0 / 1)
        self.stepper.set_reset_pose_device(pose.data_ptr(), self._ptr(mask), self._stream())
        self._keep(pose, mask)

    def _keep(self, *tensors):
        """the kernels read these when the stream gets there: they stay alive until then"""
        cur = self.torch.cuda.current_stream(self.device)
        for x in tensors:
            if x is not None:
                x.record_stream(cur)

    def _ids(self, env_ids, empty_ok=False):
        """(int32 tensor on this device or None, how many envs it names) of an `env_ids` argument (None: all envs)"""
        if env_ids is None:
            return None, self.num_envs
        t = self.torch
        ids = t.as_tensor(env_ids, dtype=t.int32, device=self.device).reshape(-1).contiguous()
        if ids.numel() < 1 and not empty_ok:
            raise ValueError("env_ids must name at least one env")
        return ids, int(ids.numel())


class DeviceVecEnv(_TensorArgs):
    def __init__(self, num_envs, device_index=0, args=None, n_modules=16, params=None, **over):
        import torch
        self.torch = torch
        self.params = params if params is not None else params_from_args(args, n_modules=n_modules, **over)
        torch.cuda.set_device(device_index)
        self.device = torch.device("cuda", device_index)
        self.stepper = _lib.Stepper(num_envs, device=device_index, params=self.params)
        self.num_envs = num_envs
        self.obs_dim = self.stepper.obs_dim
        self.act_dim = self.stepper.act_dim
        E = num_envs
        self.obs = torch.zeros((E, self.obs_dim), dtype=torch.float32, device=self.device)
        self.rew = torch.zeros((E,), dtype=torch.float32, device=self.device)
        self.done = torch.zeros((E,), dtype=torch.uint8, device=self.device)
        self.substeps = torch.zeros((E,), dtype=torch.int32, device=self.device)

    def reset(self):
        self.stepper.reset_device(0, self.obs.data_ptr(), self._stream())
        return self.obs

    def _sub_ptr(self, substeps):
        """where Snake.counter of this step goes: self.substeps, or a caller's int32 CUDA tensor [E] (a row of a per-step
        log, say: a rollout can then look at the counts after its last step instead of reducing them after every one)"""
        if substeps is None:
            return self.substeps.data_ptr()
        return self._arg(substeps, "substeps", (self.torch.int32,), (self.num_envs,), flat=True).data_ptr()

    def trace_shape(self):
        """Shape of the float32 CUDA tensor step(trace=...) fills: [E, max_counter + 1, floats per row]."""
        return self.stepper.trace_shape()

    def _trace_ptr(self, trace):
        """a caller-owned trace tensor (trace_shape(); more rows are allowed, the kernel leaves them alone)"""
        return self._arg(trace, "trace", (self.torch.float32,), self.trace_shape(), more=(1, "rows")).data_ptr()

    def _actions_ptr(self, actions):
        return self._arg(actions, "actions", (self.torch.float32,), (self.num_envs, self.act_dim)).data_ptr()

    def step(self, actions, vec_mode=True, substeps=None, trace=None):
        """actions: float32 CUDA tensor [E, A], contiguous; clipped in place.  Asynchronous.
        trace: a float32 CUDA tensor of trace_shape(): the step kernel then also writes row s of env e after its physics
        substep s, [obs | link positions | padding] (snk_step_traced); rows at and beyond the env's substep count (in
        self.substeps, or `substeps`) are not touched."""
        out = (self._actions_ptr(actions), self.obs.data_ptr(), self.rew.data_ptr(), self.done.data_ptr(),
               self._sub_ptr(substeps))
        if trace is not None:
            self.stepper.step_traced_device(*out, self._trace_ptr(trace), trace.shape[1], vec_mode, self._stream())
        else:
            self.stepper.step_device(*out, vec_mode, self._stream())
        return self.obs, self.rew, self.done

    def step_packed(self, actions, packed, vec_mode=True, substeps=None):
        """The same step, written by the kernel as rows [obs | reward | done] of `packed` ([E, >= O + 2] float32 on this
        device; the done cell holds the integer 0 / 1): the block a sharded env gathers (snk_step_packed).  self.obs /
        rew / done are NOT updated by this call.  Asynchronous."""
        self._arg(packed, "packed", (self.torch.float32,), (self.num_envs, self.obs_dim + 2), more=(1, "columns"))
        self.stepper.step_packed_device(self._actions_ptr(actions), packed.data_ptr(), packed.shape[1],
                                        self._sub_ptr(substeps), vec_mode, self._stream())
        return packed

    def set_ground_friction(self, mu):
        self.stepper.set_ground_friction(np.asarray(mu, dtype=np.float32))

    def render(self, env_ids=None, view=None, proj=None, width=128, height=96, shadow=False, depth=True, seg=True):
        """Images of the envs `env_ids` (None: all; an int32 CUDA tensor or a sequence; ids may repeat, any order) from
        their current device state, enqueued on the current stream behind the steps already there (snk_render): what
        Snake.render (snake.py:308-334) draws of one env, for any subset at once and without a host transfer.
        view / proj: column-major 16-vectors as PyBullet's computeViewMatrix* / computeProjectionMatrix* return them,
        one pair for every image or [k, 16] each (tensors or arrays); None: the [U] default camera (_lib.DEFAULT_CAMERA).
        Returns CUDA tensors (rgba [k, height, width, 4] uint8, depth [k, height, width] float32 or None, seg int32
        primitive ids or None: 0 ground, 1 + c cylinder c, 1 + 2n box, -1 background)."""
        t = self.torch
        ids, k = self._ids(env_ids, empty_ok=True)          # (the library refuses an empty list, naming the argument)
        if view is None or proj is None:
            dv, dp = _lib.default_camera(width, height)
            view, proj = (dv if view is None else view), (dp if proj is None else proj)
        v = t.as_tensor(view, dtype=t.float32, device=self.device).reshape(-1, 16)
        p = t.as_tensor(proj, dtype=t.float32, device=self.device).reshape(-1, 16)
        if v.shape[0] != p.shape[0] or v.shape[0] not in (1, k):
            raise ValueError("view / proj must be one 16-vector each or [%d, 16] each, got %s / %s"
                             % (k, tuple(v.shape), tuple(p.shape)))
        cams = t.cat([v, p], dim=1).contiguous()
        W, H = int(width), int(height)
        ok = 1 <= W <= 4096 and 1 <= H <= 4096 and k >= 1          # (the library refuses the rest, naming the argument)
        rgba = t.empty((k, H, W, 4) if ok else (4,), dtype=t.uint8, device=self.device)
        dep = t.empty((k, H, W), dtype=t.float32, device=self.device) if depth and ok else None
        sg = t.empty((k, H, W), dtype=t.int32, device=self.device) if seg and ok else None
        self.stepper.render_device(self._ptr(ids), k, cams.data_ptr(), v.shape[0] == 1, W, H,
                                   _lib.RENDER_SHADOW if shadow else 0, rgba.data_ptr(), self._ptr(dep), self._ptr(sg),
                                   self._stream())
        self._keep(ids, cams)
        return rgba, dep, sg

    def set_reset_pose(self, pose, mask=None):
        """Where the envs of `mask` (None: all) start their next episodes, at reset() and at the auto-reset inside
        step(): rows [initPosition 3 | initOrientation xyzw 4 | initState n] (snake.py:22-24, 119-127).
        A CUDA tensor [E, 7 + n] float32 (mask: None or a CUDA uint8 / bool tensor [E], e.g. the `done` a step returned)
        goes through snk_set_reset_pose_dev on the current stream: asynchronous, ordered with the steps enqueued there,
        nothing validated.  Anything else (ndarray, list, CPU tensor) goes through the host form, which synchronises and
        refuses non-finite values and non-unit quaternions."""
        t = self.torch
        if isinstance(pose, t.Tensor) and pose.is_cuda:
            # (this form takes strided views too: the copy kernel reads their contiguous copies)
            return self._reset_pose_dev(pose.contiguous(), mask.contiguous() if isinstance(mask, t.Tensor) else mask)
        if isinstance(pose, t.Tensor):
            pose = pose.numpy()
        if isinstance(mask, t.Tensor):
            mask = mask.cpu().numpy()
        self.stepper.set_reset_pose(pose, mask)

    def get_reset_pose(self):
        """[E, 7 + n] float32 ndarray: the reset-pose table (synchronises the device)."""
        return self.stepper.get_reset_pose()

    @property
    def world(self):
        """A DeviceWorld on THIS env's handle: the same environments, below the fused step."""
        if getattr(self, "_world", None) is None:
            self._world = DeviceWorld(stepper=self.stepper, device_index=self.device.index)
        return self._world

    def close(self):
        self.stepper.close()


class DeviceWorld(_TensorArgs):
    """The simulator without a task, on torch CUDA tensors: what pybullet.stepSimulation, getLinkState and
    saveState / restoreState are to a script (snake.py:219-221, 286, 138-156), for every env of a handle at once.  Every
    call is one launch on torch's current stream, ordered with what is enqueued there (a DeviceVecEnv.step or render on
    the same handle included); nothing synchronises, nothing is copied to the host.  Calls on one handle are serialised by
    the caller, as everywhere.

    DeviceWorld(num_envs, ...) owns a handle of its own; DeviceVecEnv.world shares that env's."""

    def __init__(self, num_envs=None, device_index=0, args=None, n_modules=16, params=None, stepper=None, **over):
        import torch
        self.torch = torch
        torch.cuda.set_device(device_index)
        self.device = torch.device("cuda", device_index)
        self._owns = stepper is None
        if stepper is None:
            if num_envs is None:
                raise ValueError("DeviceWorld needs num_envs (or the stepper of an existing env)")
            params = params if params is not None else params_from_args(args, n_modules=n_modules, **over)
            stepper = _lib.Stepper(num_envs, device=device_index, params=params)
        self.stepper = stepper
        self.params = stepper.params
        self.num_envs = stepper.n_envs
        self.n = stepper.n
        self.obs_dim = stepper.obs_dim
        self.link_rows = 3 * self.n + 2

    def step_simulation(self, targets, k=1, active=None, info=None):
        """k physics substeps towards the joint targets [E, n] float32 (radians): setJointMotorControlArray +
        stepSimulation (snake.py:219-221, 286).  active: uint8 / bool [E] or None (all); an env whose byte is 0 keeps
        every bit of its state.  info: int32 [E, 2] or None -- solver iterations and contact count of the last substep;
        rows of inactive envs are left alone."""
        t = self.torch
        targets = self._arg(targets, "targets", (t.float32,), (self.num_envs, self.n))
        active = self._arg(active, "active", (t.uint8, t.bool), (self.num_envs,), optional=True)   # (a bool is one byte, 0 / 1)
        info = self._arg(info, "info", (t.int32,), (self.num_envs, 2), optional=True)
        if int(k) < 0:
            raise ValueError("k must not be negative, got %d" % int(k))
        self.stepper.substep_device(targets.data_ptr(), int(k), self._ptr(active), self._ptr(info), self._stream())
        self._keep(targets, active)

    def _observe(self, which, out):
        """One snk_observe read-out, [E, ...] float32: `which` is observe_device's name of it."""
        row = {"obs_ptr": (self.obs_dim,), "height_ptr": (), "linkpos_ptr": (3 * (self.n + 1),)}[which]
        out = self._out(out, "out", (self.num_envs,) + row)
        self.stepper.observe_device(stream=self._stream(), **{which: out.data_ptr()})
        return out

    def observation(self, out=None):
        """getObservation (snake.py:209-217) of every env: [E, 3n + 8] float32."""
        return self._observe("obs_ptr", out)

    def mean_height(self, out=None):
        """checkSnakeHeight's mean z (snake.py:237-245) of every env: [E] float32."""
        return self._observe("height_ptr", out)

    def link_positions(self, out=None):
        """getLinkPositions (snake.py:138-146) of every env: [E, 3(n + 1)] float32, [x.., y.., z..] of links 0, 3, .., 3n."""
        return self._observe("linkpos_ptr", out)

    def link_states(self, env_ids=None, out=None):
        """[k, 3n + 2, 16] float32: getLinkState(computeLinkVelocity=1) of every link of the envs `env_ids` (None: all;
        an int32 CUDA tensor or a sequence; ids may repeat, any order; an id outside the handle gives zero rows).  Row r
        is Bullet link r - 1 (row 0: the root); a row is [COM 3 | quaternion xyzw 4 | link-frame origin 3 | COM velocity
        3 | angular velocity 3], world frame."""
        ids, k = self._ids(env_ids)
        out = self._out(out, "out", (k, self.link_rows, _lib.LINK_STATE_FLOATS))
        self.stepper.link_states_device(self._ptr(ids), k, out.data_ptr(), self._stream())
        self._keep(ids)
        return out

    def contacts(self, env_ids=None, out=None):
        """(points [k, slots, 16] float32, force [k, 2n + 1] float32, count [k] int32): the ground contacts of the envs
        `env_ids` (None: all; an int32 CUDA tensor or a sequence; ids may repeat, any order; an id outside the handle gives
        zeros), read from the contact cache at the current pose by one launch (snk_contacts; include/snk.h has the
        contract).  Slot 4 c + j is cached point j of cylinder c, the last four of an obstacle 2 world the free box's; a
        slot is [point on the body 3 | point on the ground 3 | normal 3 | distance | normal force N | impulse | c (2n: the
        box) | j | live | 0], zeros when not live.  out: a (points, force, count) tuple of tensors to write into."""
        po, fo, co = (None, None, None) if out is None else out
        return self._contacts(env_ids, ("out[0]", po), ("out[1]", fo), ("out[2]", co))

    def _contacts(self, env_ids, points=None, force=None, count=None):
        """One snk_contacts launch for the outputs wanted (_want)."""
        ids, k = self._ids(env_ids)
        # (contact_slots is asked only with the records: contact_forces leaves a contact_model 0 handle to snk_contacts' refusal)
        points = points and self._want(points, (k, self.stepper.contact_slots, _lib.CONTACT_FLOATS))
        force = self._want(force, (k, 2 * self.n + 1))
        count = self._want(count, (k,), self.torch.int32)
        self.stepper.contacts_device(self._ptr(ids), k, self._ptr(points), self._ptr(force), self._ptr(count), self._stream())
        self._keep(ids)
        return points, force, count

    def contact_forces(self, out=None):
        """[E, 2n + 1] float32: the normal force of the ground on every cylinder of every env, in newtons (entry 2n: on
        the free box, 0 without one) -- the touch / ground-reaction term of a reward written over step_simulation."""
        return self._contacts(None, force=("out", out))[1]

    def closest_points(self, distance, env_ids=None, flags=_lib.PAIRS_BOX | _lib.PAIRS_LINKS, max_pairs=64, out=None):
        """(points [k, 2n + max_pairs, 16] float32, clearance [k, 2, 2n] float32, count [k, 2] int32): PyBullet's
        getClosestPoints(snake, block, distance) and (snake, snake, distance) of the envs `env_ids` (None: all; an int32
        CUDA tensor or a sequence; ids may repeat, any order; an id outside the handle gives zeros), the solver's narrow
        phase run as a query on the current pose by one launch (snk_closest_points; include/snk.h has the contract).  Slot
        c < 2n is the pair (cylinder c, box); the found link-link pairs follow, compact, in the solver's order, the first
        `max_pairs` of them.  A slot is [point on cylinder a 3 | point on B 3 | normal on B 3 | distance | tier | 0 | a |
        b (2n: the box) | live | 0], zeros when not live; count[:, 1] is not clipped to max_pairs.  out: a (points,
        clearance, count) tuple of tensors to write into."""
        po, co, no = (None, None, None) if out is None else out
        return self._closest(distance, env_ids, flags, max_pairs, ("out[0]", po), ("out[1]", co), ("out[2]", no))

    def _closest(self, distance, env_ids, flags, max_pairs, points=None, clearance=None, count=None):
        """One snk_closest_points launch for the outputs wanted (_want)."""
        ids, k = self._ids(env_ids)
        points = points and self._want(points, (k, self.stepper.closest_slots(max_pairs), _lib.CONTACT_FLOATS))
        clearance = self._want(clearance, (k, 2, 2 * self.n))
        count = self._want(count, (k, 2), self.torch.int32)
        self.stepper.closest_points_device(self._ptr(ids), k, distance, flags, max_pairs, self._ptr(points),
                                           self._ptr(clearance), self._ptr(count), self._stream())
        self._keep(ids)
        return points, clearance, count

    def clearance(self, distance, flags=_lib.PAIRS_BOX | _lib.PAIRS_LINKS, out=None):
        """[E, 2, 2n] float32: per cylinder of every env its distance to the box (row 0) and to the nearest other link it
        forms a pair with (row 1), each min(found distances, distance) -- `distance` reads "nothing within reach".  The
        proximity term of a reward written over step_simulation; no records are written."""
        return self._closest(distance, None, flags, 0, clearance=("out", out))[1]

    def ray_test(self, rays, env_ids=None, parent_row=-1, flags=_lib.RAYS_ALL, out=None):
        """[k, R, 8] float32: PyBullet's rayTestBatch for the envs `env_ids` (None: all; an int32 CUDA tensor or a sequence;
        ids may repeat, any order; every ray of an id outside the handle misses), cast at the current pose by two launches
        (snk_ray_test; include/snk.h has the contract).  rays: a float32 CUDA tensor [k, R, 6], [from 3 | to 3] per ray --
        torch.cat((from, to), -1) -- or [R, 6]: one fan for every row.  parent_row -1: world coordinates; r: the frame of
        row r of link_states of the row's own env (origin the link's COM; PyBullet's parentLinkIndex L is row L + 1).
        flags: RAYS_GROUND | RAYS_SNAKE | RAYS_BOX, what can be hit.  A record is [hit fraction | position 3 | outward
        normal 3 | primitive id: 0 ground, 1 + c cylinder c, 1 + 2n the box], world frame; a miss is [1, 0 x 6, -1]."""
        t = self.torch
        ids, k = self._ids(env_ids)
        if not isinstance(rays, t.Tensor) or rays.dim() not in (2, 3) or rays.shape[-1] != _lib.RAY_FLOATS or rays.shape[-2] < 1:
            raise ValueError("rays must be a CUDA tensor [%d, R, 6] or [R, 6]" % k)
        shared = rays.dim() == 2
        R = int(rays.shape[-2])
        rays = self._arg(rays, "rays", (t.float32,), (R, _lib.RAY_FLOATS) if shared else (k, R, _lib.RAY_FLOATS))
        out = self._out(out, "out", (k, R, _lib.HIT_FLOATS))
        self.stepper.ray_test_device(self._ptr(ids), k, rays.data_ptr(), R, parent_row,
                                     (int(flags) & ~_lib.RAYS_SHARED) | (_lib.RAYS_SHARED if shared else 0), out.data_ptr(),
                                     self._stream())
        self._keep(ids, rays)
        return out

    def ranges(self, rays, env_ids=None, parent_row=-1, flags=_lib.RAYS_ALL):
        """[k, R] float32: the range along every ray of ray_test, hit fraction x |to - from| in metres -- the ray's own
        length where nothing is hit.  The reading of a range sensor riding on link row `parent_row`."""
        hits = self.ray_test(rays, env_ids, parent_row, flags)
        return hits[..., 0] * (rays[..., 3:6] - rays[..., 0:3]).norm(dim=-1)

    def dynamics(self, env_ids=None, gravity=True, velocity=True, out=None):
        """(M [k, nd, nd] float32, h [k, nd] float32), nd = 6 + n: the joint-space inertia and the bias forces of the envs
        `env_ids` (None: all; an int32 CUDA tensor or a sequence; ids may repeat, any order; an id outside the handle gives
        zeros) at the state they hold, by one launch (snk_dynamics; include/snk.h has the contract): M du/dt + h = Q over
        u = [omega 3 | v of the root origin 3 | qd n] -- PyBullet's calculateMassMatrix and calculateInverseDynamics(q, qd,
        0).  gravity / velocity: the terms of h.  out: an (M, h) tuple of tensors to write into."""
        mo, ho = (None, None) if out is None else out
        return self._dynamics(env_ids, self._bias_flags(gravity, velocity), ("out[0]", mo), ("out[1]", ho))

    def _dynamics(self, env_ids, flags, M=None, h=None):
        """One snk_dynamics launch for the outputs wanted (_want)."""
        ids, k = self._ids(env_ids)
        nd = self.n + 6
        M = self._want(M, (k, nd, nd))
        h = self._want(h, (k, nd))
        self.stepper.dynamics_device(self._ptr(ids), k, flags, self._ptr(M), self._ptr(h), self._stream())
        self._keep(ids)
        return M, h

    @staticmethod
    def _bias_flags(gravity, velocity):
        flags = (_lib.BIAS_GRAVITY if gravity else 0) | (_lib.BIAS_VELOCITY if velocity else 0)
        if not flags:
            raise ValueError("bias forces need gravity, velocity or both")
        return flags

    def mass_matrix(self, env_ids=None, out=None):
        """[k, nd, nd] float32: M(q) alone (dynamics' first output), symmetric bit for bit; 1/2 u^T M u is the kinetic
        energy."""
        return self._dynamics(env_ids, _lib.BIAS_VELOCITY | _lib.BIAS_GRAVITY, M=("out", out))[0]

    def bias_forces(self, env_ids=None, gravity=True, velocity=True, out=None):
        """[k, nd] float32: h alone (dynamics' second output): the Coriolis, centrifugal and gyroscopic forces at the
        state's u (`velocity`) minus the generalised gravity force (`gravity`); gravity alone is what a controller adds to
        hold the pose.  Rigid bodies only: none of the integrator's damping."""
        return self._dynamics(env_ids, self._bias_flags(gravity, velocity), h=("out", out))[1]

    def jacobians(self, link_rows, local=None, env_ids=None, out=None):
        """[k, P, 6, nd] float32: PyBullet's calculateJacobian for P points of the envs `env_ids` (None: all; an int32 CUDA
        tensor or a sequence; ids may repeat, any order; an id outside the handle gives zeros), by one launch
        (snk_jacobians).  link_rows: P rows of link_states (Bullet link + 1), a list or an int32 tensor, shared by every
        env; local: [P, 3] float32 points in the links' COM frames, a list or a tensor (None: the COMs).  Rows 0-2: the
        point's world velocity per unit of each component of u; rows 3-5: the link's angular velocity.  A link row outside
        0 .. 3n + 1 gives a zero Jacobian."""
        t = self.torch
        ids, k = self._ids(env_ids)
        rows = t.as_tensor(link_rows, dtype=t.int32, device=self.device).reshape(-1).contiguous()
        P = int(rows.numel())
        if not 1 <= P <= _lib.JAC_MAX_POINTS:
            raise ValueError("link_rows must name 1 .. %d points, got %d" % (_lib.JAC_MAX_POINTS, P))
        loc = None
        if local is not None:
            loc = t.as_tensor(local, device=self.device)
            if loc.dtype != t.float32 and isinstance(local, t.Tensor):
                raise ValueError("local must be torch.float32, got %s" % loc.dtype)
            loc = loc.to(t.float32)
            if tuple(loc.shape) != (P, 3):
                raise ValueError("local must have shape %s, got %s" % ((P, 3), tuple(loc.shape)))
            loc = loc.contiguous()
        out = self._out(out, "out", (k, P, 6, self.n + 6))
        self.stepper.jacobians_device(self._ptr(ids), k, rows.data_ptr(), self._ptr(loc), P, out.data_ptr(), self._stream())
        self._keep(ids, rows, loc)
        return out

    def apply_forces(self, gen_force=None, link_rows=None, wrenches=None, frame="world", duration=None, active=None,
                     dry=False, out=None):
        """Applies forces for `duration` seconds to the state as it lies: the velocity u of every active env becomes u +
        delta, delta = duration x M(q)^-1 Q, by one launch in front of whatever steps next (snk_apply_impulse; include/snk.h,
        "The applied forces") -- PyBullet's applyExternalForce / applyExternalTorque and, with max_motor_impulse=0,
        TORQUE_CONTROL.  Q = gen_force + sum over the points of J^T [force ; torque], J what jacobians() reports:
        gen_force  [E, nd] float32 or None: moment about the root origin 3 | force 3 | joint torques n (conjugate to u)
        link_rows  P rows of link_states (Bullet link + 1), a list or an int32 tensor, shared by every env; 0 .. 256 of them
        wrenches   [E, P, 9] float32: [force 3 | torque 3 | point 3] per env and point
        frame      "world": world axes and a world point (WORLD_FRAME); "link": the link's COM frame (LINK_FRAME)
        duration   seconds the forces are held (None: the handle's dt as the kernels hold it)
        active     uint8 / bool [E] or None (all): an env whose byte is 0 keeps every bit of its state; its delta is zeros
        dry        nothing is written: delta alone (impulse_response)
        Returns `out` ([E, nd] float32: delta) when given or when dry, else None."""
        t = self.torch
        nd = self.n + 6
        if frame not in ("world", "link"):
            raise ValueError("frame must be 'world' or 'link', got %r" % (frame,))
        gen_force = self._arg(gen_force, "gen_force", (t.float32,), (self.num_envs, nd), optional=True)
        rows = None
        P = 0
        if link_rows is not None:
            rows = t.as_tensor(link_rows, dtype=t.int32, device=self.device).reshape(-1).contiguous()
            P = int(rows.numel())
        if P > _lib.IMPULSE_MAX_POINTS:
            raise ValueError("link_rows must name 0 .. %d points, got %d" % (_lib.IMPULSE_MAX_POINTS, P))
        if P or wrenches is not None:
            if wrenches is None:
                raise ValueError("link_rows without wrenches")
            wrenches = self._arg(wrenches, "wrenches", (t.float32,), (self.num_envs, P, _lib.WRENCH_FLOATS))
        if gen_force is None and P == 0:
            raise ValueError("nothing to apply: neither gen_force nor wrenches")
        active = self._arg(active, "active", (t.uint8, t.bool), (self.num_envs,), optional=True)
        if dry or out is not None:
            out = self._out(out, "out", (self.num_envs, nd))
        seconds = float(np.float32(self.params.dt)) if duration is None else float(duration)
        flags = (_lib.IMPULSE_LINK_FRAME if frame == "link" else 0) | (_lib.IMPULSE_DRY if dry else 0)
        self.stepper.apply_impulse_device(self._ptr(active), self._ptr(gen_force), self._ptr(rows if P else None),
                                          self._ptr(wrenches if P else None), P, flags, seconds, self._ptr(out),
                                          self._stream())
        self._keep(active, gen_force, rows, wrenches)
        return out

    def impulse_response(self, gen_force=None, link_rows=None, wrenches=None, frame="world", duration=None, active=None,
                         out=None):
        """[E, nd] float32: M(q)^-1 Q x duration of apply_forces' arguments, with nothing of the state written (its dry
        form): what the forces WOULD do to u."""
        return self.apply_forces(gen_force, link_rows, wrenches, frame, duration, active, dry=True, out=out)

    def reset(self, mask=None, out=None):
        """The soft reset (snake.py:96-99, 119-127) of the envs of `mask` (uint8 / bool [E]; None: all) onto their rows
        of the reset-pose table.  Returns the observations [E, 3n + 8]; rows of unmasked envs are left as `out` had them
        (zeros for a fresh tensor)."""
        t = self.torch
        mask = self._arg(mask, "mask", (t.uint8, t.bool), (self.num_envs,), optional=True)
        if out is None:
            out = t.zeros((self.num_envs, self.obs_dim), dtype=t.float32, device=self.device)
        else:
            out = self._arg(out, "out", (t.float32,), (self.num_envs, self.obs_dim))
        self.stepper.reset_device(self._ptr(mask), out.data_ptr(), self._stream())
        self._keep(mask)
        return out

    def set_reset_pose(self, pose, mask=None):
        """Rows [position 3 | quaternion xyzw 4 | joint angles n] of the reset-pose table from CUDA tensors (pose [E, 7 +
        n] float32, mask uint8 / bool [E] or None): snk_set_reset_pose_dev on the current stream, nothing validated."""
        self._reset_pose_dev(pose, mask)

    def fork(self, src, dst, reset_pose=False):
        """Env dst[i] becomes env src[i] in everything a Snapshot holds: state record, contact cache, free box, ground
        friction -- and with reset_pose=True its row of the reset-pose table.
        Host lists / arrays are VALIDATED (ids inside the handle, the dst ids distinct, no env on both sides; a ValueError
        names the index) and then uploaded.  int32 CUDA tensors go to the kernel as they are, UNVALIDATED, without a
        host round trip: the caller keeps that contract; broken, which copy wins is undefined and an id outside the
        handle makes its pair a no-op."""
        t = self.torch
        if isinstance(src, t.Tensor) and src.is_cuda and isinstance(dst, t.Tensor) and dst.is_cuda:
            k = int(src.numel())
            s = self._arg(src.reshape(-1), "src", (t.int32,), (k,))
            d = self._arg(dst.reshape(-1), "dst", (t.int32,), (k,))
        else:
            hs = np.asarray(src.cpu() if isinstance(src, t.Tensor) else src).reshape(-1)
            hd = np.asarray(dst.cpu() if isinstance(dst, t.Tensor) else dst).reshape(-1)
            check_fork_ids(hs, hd, self.num_envs)
            s = t.as_tensor(hs.astype(np.int32), device=self.device)
            d = t.as_tensor(hd.astype(np.int32), device=self.device)
        if s.numel() < 1:
            raise ValueError("fork needs at least one (src, dst) pair")
        self.stepper.copy_envs_device(s.data_ptr(), d.data_ptr(), int(s.numel()), reset_pose, self._stream())
        self._keep(s, d)

    def close(self):
        if self._owns:
            self.stepper.close()


def check_fork_ids(src, dst, num_envs):
    """snk_copy_envs' contract on host id lists (what snk_copy_envs_host refuses): raises ValueError naming the index."""
    if len(src) != len(dst):
        raise ValueError("src and dst must name as many envs each, got %d and %d" % (len(src), len(dst)))
    for name, ids in (("src", src), ("dst", dst)):
        for i, e in enumerate(ids):
            if int(e) != e or not 0 <= int(e) < num_envs:
                raise ValueError("%s[%d] = %s is outside 0 .. %d" % (name, i, e, num_envs - 1))
    first = {}
    for i, e in enumerate(dst):
        if int(e) in first:
            raise ValueError("dst[%d] = %d repeats dst[%d] (the destinations must be distinct)" % (i, int(e), first[int(e)]))
        first[int(e)] = i
    sources = {int(e): i for i, e in reversed(list(enumerate(src)))}
    for i, e in enumerate(dst):
        if int(e) in sources:
            raise ValueError("dst[%d] = %d is also src[%d] (no env may be both a source and a destination)"
                             % (i, int(e), sources[int(e)]))


class ShardedVecEnv(object):
    """Envs sharded over the ranks of a process group; SubprocVecEnv API on the root rank.

    local_env: object with num_envs, obs_dim, act_dim, reset() -> obs tensor [E,O], and either
               step_packed(actions tensor [E,A], packed tensor [E,O+2]) writing rows [obs | reward | done] into
               `packed` itself (DeviceVecEnv: the step kernel does; the done cell holds the INTEGER 0 / 1, i.e. its
               int32 bits inside the float32 block) -- or, without that method, the plain
               step(actions) -> (obs [E,O], rew [E], done [E]) on `device`, whose results are then copied into the block.
    Every rank must call reset()/step() collectively; non-root ranks pass actions=None and get
    (None, None, None, ()) back.
    fresh_infos: True = a fresh dict per env per step, as the reference's workers send (32 768 dicts cost the root of 8
    ranks about 1 ms of every step); False (default) = one read-only, picklable FrozenInfo repeated.
    """

    def __init__(self, local_env, root=0, group=None, device=None, fresh_infos=False):
        import torch
        import torch.distributed as dist
        self.torch, self.dist = torch, dist
        self.env = local_env
        self.group = group
        self.rank = dist.get_rank(group)
        self.world = dist.get_world_size(group)
        self.root = root
        self.device = device if device is not None else getattr(local_env, "device", torch.device("cpu"))
        self.E = local_env.num_envs
        self.O = local_env.obs_dim
        self.A = local_env.act_dim
        self.num_envs = self.E * self.world
        self.backend = dist.get_backend(group)
        # The collectives run where the backend can: on the device for "nccl" (RCCL over xGMI), through host
        # staging for "gloo" (CPU tests; rehearsing a multi-rank run on a box with one GPU).
        self._xdev = self.device if dist.get_backend(group) == "nccl" else torch.device("cpu")
        self._act = torch.zeros((self.E, self.A), dtype=torch.float32, device=self._xdev)
        self._pack = torch.zeros((self.E, self.O + 2), dtype=torch.float32, device=self.device)
        if self.rank == root:
            # one preallocated [world * E, O + 2] buffer; the gather writes each rank's block into its slice
            self._all = torch.zeros((self.num_envs, self.O + 2), dtype=torch.float32, device=self._xdev)
            self._gather_list = list(self._all.split(self.E, dim=0))
            self._all_dev = self._all if self._xdev == self.device else torch.zeros_like(self._all, device=self.device)
            self._act_all = torch.zeros((self.num_envs, self.A), dtype=torch.float32, device=self._xdev)
        else:
            self._gather_list = None
        self._infos = None if fresh_infos else (FrozenInfo(),) * self.num_envs
        self._packed_step = hasattr(local_env, "step_packed")

    def __len__(self):
        return self.num_envs

    def shard_slice(self, rank=None):
        r = self.rank if rank is None else rank
        return slice(r * self.E, (r + 1) * self.E)

    def _gather(self):
        """self._pack (this rank's [E, O + 2] block) -> the root's [world * E, O + 2] buffer: the ONE collective of the
        return path (ppo/multiprocessing_env.py:125-128 is a recv per worker)."""
        self.dist.gather(self._pack if self._xdev == self.device else self._pack.to(self._xdev), self._gather_list,
                         dst=self.root, group=self.group)
        if self.rank != self.root:
            return None
        if self._all_dev is not self._all:
            self._all_dev.copy_(self._all)
        return self._all_dev

    def reset(self):
        # (a reset is once per run, not per step: the observation is copied into the block's first O columns)
        self._pack[:, :self.O] = self.env.reset()
        self._pack[:, self.O:] = 0
        allp = self._gather()
        return None if allp is None else allp[:, :self.O]

    def step(self, actions=None):
        """The root's `actions` (tensor or ndarray [world * E, A] or [.., A, 1]) are NOT modified: SubprocVecEnv pickles
        them to its workers (ppo/multiprocessing_env.py:119-122), so checkBound (SnakeGymEnv.py:82-88) only ever clips
        the workers' copies -- here the scattered copies, which the step kernels clip.
        Returns VIEWS of the gathered block (obs [:, :O], reward [:, O], done from the integer cell [:, O + 1]); a
        caller that moves the results on (to the host, into a rollout buffer) should take step_block() and move the
        contiguous block in one copy."""
        t = self.torch
        allp = self.step_block(actions)
        if allp is None:
            return None, None, None, ()
        infos = self._infos if self._infos is not None else tuple({} for _ in range(self.num_envs))
        # the done cell holds the integer 0 / 1 (its bits travel in the float32 block)
        return allp[:, :self.O], allp[:, self.O], allp.view(t.int32)[:, self.O + 1] != 0, infos

    def step_block(self, actions=None, substeps=None):
        """One collective env-step; on the root returns the contiguous [world * E, O + 2] float32 block on `device`
        (rows [obs | reward | done as int32 bits], env g in row g), None elsewhere.  Valid until the next call."""
        t = self.torch
        if self.rank == self.root:
            a = t.as_tensor(actions, dtype=t.float32)       # shares memory with a float32 ndarray / tensor
            a2 = a[:, :, 0] if (a.dim() == 3 and a.shape[2] == 1) else a
            if tuple(a2.shape) != (self.num_envs, self.A):
                raise _lib._ArgError("actions must have shape %s, got %s" % ((self.num_envs, self.A), tuple(a2.shape)))
            self._act_all.copy_(a2, non_blocking=True)      # (asynchronous only from pinned host memory / the device)
            chunks = list(self._act_all.split(self.E, dim=0))
        else:
            a2 = None
            chunks = None
        self.dist.scatter(self._act, chunks, src=self.root, group=self.group)
        # the local env writes its rows [obs | reward | done] into the block itself (DeviceVecEnv: the step kernel does,
        # snk_step_packed): nothing is copied between the physics and the gather
        a_loc = self._act if self._xdev == self.device else self._act.to(self.device)
        if self._packed_step:
            # (substeps: where the local env's substep counts of this step go -- DeviceVecEnv.step_packed's argument)
            if substeps is not None:
                self.env.step_packed(a_loc, self._pack, substeps=substeps)
            else:
                self.env.step_packed(a_loc, self._pack)
        else:
            # a local env with the plain contract: its results copied into the block (three small copies per step)
            obs, rew, done = self.env.step(a_loc)
            self._pack[:, :self.O] = obs
            self._pack[:, self.O] = rew
            self._pack.view(t.int32)[:, self.O + 1] = (t.as_tensor(done) != 0).to(t.int32)
        return self._gather()

    def set_reset_pose(self, pose, mask=None):
        """Every rank calls this with the GLOBAL arrays, pose [world * E, 7 + n] and mask [world * E] or None (host
        data: ndarray or CPU tensor), and hands its own slice (shard_slice) to its local env through the host form.  No
        communication: like set_ground_friction on the local envs, the data is the caller's on every rank."""
        t = self.torch
        pose = pose.cpu().numpy() if isinstance(pose, t.Tensor) else np.asarray(pose, dtype=np.float32)
        if pose.ndim != 2 or pose.shape[0] != self.num_envs:
            raise ValueError("reset pose must have %d rows (all ranks' envs), got shape %s" % (self.num_envs, pose.shape))
        sl = self.shard_slice()
        if mask is not None:
            mask = mask.cpu().numpy() if isinstance(mask, t.Tensor) else np.asarray(mask)
            if mask.shape != (self.num_envs,):
                raise ValueError("mask must have shape (%d,), got %s" % (self.num_envs, mask.shape))
            mask = mask[sl]
        self.env.set_reset_pose(np.ascontiguousarray(pose[sl]), mask)

    def close(self):
        if hasattr(self.env, "close"):
            self.env.close()
