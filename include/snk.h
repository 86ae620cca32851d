/*
 * snk.h -- C ABI of the MI355X batched snake stepper (libsnk.so).
 *
 * Drop-in boundary for ONE path of vinits5/bullet-envs: SnakeGymEnv.step()/reset(),
 * whose arithmetic the reference delegates to pybullet.stepSimulation on the CPU.
 * Everything here is plain C: pointers, sizes, int status codes; no torch types.
 * Paths cited below are under /root/reference.
 *
 * One handle = N independent environments resident on one GPU.  Calls on a handle
 * are serialised by the caller (the reference is single-threaded per env process,
 * multiprocessing_env.py:7-29).  Functions return 0 on success, non-zero on error;
 * snk_last_error() gives the message.  No exceptions cross this boundary.
 */
#ifndef SNK_H
#define SNK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Every knob the reference path depends on.  [U] = PyBullet/Bullet default taken from
 * knowledge of bullet3 (not verifiable here). */
#define SNK_ABI_VERSION 7       /* bumped whenever snk_params' layout or an entry point's meaning changes */

typedef struct snk_params {
    /* layout guard (round 6): snk_default_params fills both, snk_create refuses a struct whose size or
       version is not this library's -- a caller compiled against another header gets an error message, not garbage
       parameters.  New fields are appended at the END of the struct from here on. */
    uint32_t struct_size;       /* sizeof(snk_params) of the header the caller was compiled against */
    uint32_t abi_version;       /* SNK_ABI_VERSION of that header                                    */
    /* model: snake/snake.urdf (constants generated parametrically, not parsed) */
    int32_t n_modules;          /* 16 = snake.urdf; 32 = BASELINE config 4 (only these two)      */
    int32_t inertia_from_file;  /* 0: inertia from collision AABB [U] (snake.py:93 passes no
                                   URDF_USE_INERTIA_FROM_FILE); 1: urdf:815,871 values       */
    double  default_mass;       /* links without <inertial> (urdf:7,14,818): mass 1 [U]       */
    double  collision_margin;   /* 0.001 [U]                                                  */
    int32_t hull_sides;         /* 32 (default): the 32-gon prism PyBullet builds for a URDF <cylinder> unless
                                   URDF_USE_IMPLICIT_CYLINDER [U] (snake.py:93 passes no such flag); 0: implicit
                                   cylinder (the round-1 model); 0 or 3..32                           */
    int32_t contact_model;      /* 1 (default): Bullet's persistent manifold [U] -- one new support point per
                                   cylinder per step merged into a cache of <= 4, refreshed / dropped at the
                                   breaking threshold; 0: stateless -- both end-cap points of
                                   every cylinder, every step (the round-1 model)                      */
    int32_t self_collision;     /* 1 (default): link-link contacts between non-adjacent cylinder links, what
                                   URDF_USE_SELF_COLLISION (snake.py:93) switches on [U].  Their two-body rows are
                                   built by the streamed-row solve; a 16-link substep in which some pair of links may
                                   be within the breaking threshold goes through it (never inside the reference's
                                   command range)                                              */
    int32_t obstacle;           /* the box of snake/block.urdf that Snake.add_obstacle (snake.py:83-84, commented out
                                   at :94) and snake_gait_test.py:51 put in front of the snake.  0 (default): none.
                                   1: STATIC (16 links: up to 8 contacts with it, out of the solve's 64 slots).
                                   2: as the reference loads it (useFixedBase=0): a FREE body of obstacle_mass resting
                                   on the ground -- its own six velocity components, gravity, damping, a persistent
                                   manifold with the plane, two-body rows with the snake's links; 16 links only, on
                                   the streamed-row kernels                                       */
    double  obstacle_pos[3];    /* centre of the box: [2, 0, 0.1] (snake.py:94, snake_gait_test.py:51)         */
    double  obstacle_half[3];   /* half extents: [0.1, 0.4, 0.1] (snake/block.urdf:16)                         */
    double  mu_obstacle;        /* 0.5 [U]: Bullet's default lateral friction for a link without <contact>     */
    double  obstacle_mass;      /* 200 (snake/block.urdf:6); inertia from the box shape [U] (inertia_from_file 1:
                                   block.urdf:7's 1, 100, 1)                                                   */
    /* pybullet world */
    double  dt;                 /* 1/240 [U]: setTimeSteps is never called (snake.py:271-272) */
    double  gravity_z;          /* snake.py:8,91   -9.8                                       */
    double  lin_damping;        /* 0.04 [U]                                                   */
    double  ang_damping;        /* 0.04 [U]                                                   */
    double  joint_damping;      /* snake.urdf:838  0.1                                        */
    double  max_coord_vel;      /* 100 [U]                                                    */
    /* setJointMotorControlArray(POSITION_CONTROL) defaults, snake.py:219-221 */
    double  kp;                 /* 0.1 [U]                                                    */
    double  kd;                 /* 1.0 [U]                                                    */
    double  max_motor_impulse;  /* forces=[inf] (snake.py:26-27) -> +inf                      */
    double  joint_lo, joint_hi; /* snake.urdf:839  -1.57, 1.57                                */
    double  limit_erp;          /* 0.2 [U]                                                    */
    double  limit_max_impulse;  /* 100 [U]                                                    */
    /* changeDynamics, snake.py:103-107 */
    double  mu_link;            /* lateralFriction = 2                                        */
    double  aniso[3];           /* anisotropicFriction = [1, 0.1, 0.01] (snake.py:25)         */
    double  contact_erp;        /* 0.08 [U]                                                   */
    double  linear_slop;        /* 1e-5 [U]                                                   */
    double  breaking_threshold; /* 0.02 [U] gContactBreakingThreshold                         */
    int32_t relative_breaking_threshold; /* 1 (default) [U]: btCollisionDispatcher's default flag
                                   CD_USE_RELATIVE_CONTACT_BREAKING_THRESHOLD -- a manifold's threshold is
                                   breaking_threshold x the smaller angular-motion disc of its two shapes, computed
                                   from the link collider's AABB (0.0603 m -> 1.206 mm); 0: breaking_threshold itself */
    int32_t cone_friction;      /* 1 [U]                                                      */
    int32_t n_iterations;       /* 50 [U]                                                     */
    double  residual_threshold; /* 1e-7 [U]; 0 disables the early exit                        */
    int32_t warm_start;         /* 0 (default) [U]: btMultiBodyConstraintSolver::setupMultiBodyContactConstraint has its
                                   warm start disabled, every row starts at zero impulse.  1: SOLVER_USE_WARMSTARTING as
                                   the rigid-body solver does it -- a cached point's normal row starts at
                                   warmstarting_factor x the impulse it carried in the last substep (the contact cache
                                   keeps it: btManifoldPoint::m_appliedImpulse), delta-v at the sum of M^-1 J^T of those;
                                   friction rows start at zero.  Needs contact_model 1                            */
    double  warmstarting_factor;/* 0.85 [U] btContactSolverInfo::m_warmstartingFactor            */
    int32_t friction_directions;/* 2 (default) [U]: SOLVER_USE_2_FRICTION_DIRECTIONS -- both btPlaneSpace1 tangents of a
                                   contact get a friction row (with cone_friction: the implicit cone over the pair).
                                   1: Bullet's multibody solver WITHOUT that flag -- one row per contact, along the first
                                   tangent ((0,-1,0) for the ground's normal), bounds +-mu lambda_n.  A switch since
                                   round 5 because the oracle prices it above the error bar's other rows (+14 % forward
                                   motion under the bench gait: profiles/r05_u_rows.json); the default is the reading
                                   under which a body pushed along world x comes to rest, as it does in PyBullet      */
    /* Snake / SnakeGymEnv */
    double  scaling_factor;     /* snake.py:63   pi/6                                         */
    int32_t gait;               /* snake.py:62   1: actions drive odd motor slots             */
    double  servo_tol;          /* snake.py:232  0.05                                         */
    int32_t max_counter;        /* snake.py:303  40  (=> at most 41 substeps)                 */
    double  height_threshold;   /* snake.py:238  0.1                                          */
    double  energy_dt;          /* snake.py:9,339  1/100                                      */
    double  alpha, beta, gamma; /* SnakeGymEnv.py:14-16  1, 0.01, 0.1                         */
    double  term_angle;         /* SnakeGymEnv.py:100  0.5                                    */
    int32_t term_index;         /* SnakeGymEnv.py:100  obs index 9                            */
    double  collision_force;    /* SnakeGymEnv.py:94   10                                     */
    double  collision_penalty;  /* SnakeGymEnv.py:94   -10                                    */
    double  done_penalty;       /* SnakeGymEnv.py:40   -5                                     */
    /* (appended in round 6: new fields go to the END of the struct) */
    int32_t contact_order;      /* 0 (default): the solver sweeps the ground manifolds in link order.  [U]: Bullet hands its
                                   solver the manifolds in the island manager's order, which is not knowable here, and
                                   with 50 unconverged sweeps the order is part of the answer -- the oracle prices other
                                   orders at -3 % .. -24 % of forward motion under the bench gait, the largest entry of
                                   the error bar (profiles/r06_u_rows.json), hence a switch: 1 = link order reversed;
                                   2 = link order after the island manager's unstable quickSort on equal island ids (the
                                   one candidate that can be restated: btAlignedObjectArray::quickSort over the 2n plane-link
                                   manifolds); k >= 3 = the fixed permutation of the cylinder links that sorting by a hash
                                   of (k, link) gives (the same every substep, as a list of persistent manifolds keeps its
                                   order).  A
                                   cylinder's <= 4 points stay together and in their own order.  Needs contact_model 1 */
    int32_t reserved0;          /* 0 */
    /* (appended with ABI 7: two solver rules that the oracle alone had before) */
    int32_t noncontact_order;   /* 0 (default): the violated joint limits by joint index, then the n motors by joint index.
                                   1: the order btMultiBodyDynamicsWorld::solveConstraints is read to hand its solver [U] --
                                   the world's list [limit_1..limit_n, motor_1..motor_n] after btAlignedObjectArray::quickSort
                                   on equal island ids, which is not stable: its first partition reverses the list, so the n
                                   motors come first, then the violated limits, both in one fixed non-identity pattern
                                   (snk_debug_noncontact_order).  The oracle prices it at +0.3 % of forward motion under the
                                   bench gait, -23.4 % together with contact_order 2 (profiles/r06_u_rows.json)        */
    int32_t contact_erp_rule;   /* 0 (default): a penetrating contact row takes contact_erp (m_erp2, 0.08) at any depth.
                                   1: the choice setupMultiBodyContactConstraint is read to make [U]: limit_erp (m_erp, 0.2)
                                   unless split impulse is on and the contact is deeper than
                                   m_splitImpulsePenetrationThreshold (-0.04 m), only then contact_erp.  Ground, link-link
                                   and box contacts alike.  The oracle prices it at -0.5 % of forward motion             */
} snk_params;

typedef struct snk_handle snk_handle;

/* Fills the reference's defaults (Snake.defaultParams snake.py:55-63, SnakeGymEnv.py:13-17). */
void snk_default_params(snk_params* p);

/* Replaces: Snake.__init__ + SnakeGymEnv.__init__ -> robot.reset(hardReset=True)
 * (snake.py:14-32,88-95; SnakeGymEnv.py:5-26) for n_envs worlds at once, and the N worker
 * processes of SubprocVecEnv.__init__ (ppo/multiprocessing_env.py:97-117).
 * device = HIP device ordinal.  State after create = hard reset. */
int snk_create(const snk_params* p, int32_t n_envs, int32_t device, snk_handle** out);
int snk_destroy(snk_handle* h);

int32_t snk_num_envs(const snk_handle* h);
int32_t snk_obs_dim(const snk_handle* h);    /* 3n+8  (snake.py:163-164)            */
int32_t snk_act_dim(const snk_handle* h);    /* n/2 for gait 0/1 (SnakeGymEnv.py:74-76) */
int32_t snk_state_dim(const snk_handle* h);  /* 13+2n: pos3 quat_xyzw4 omega3 vel3 q qd */
int32_t snk_record_floats(const snk_handle* h); /* floats per env in the HBM state record */

/* Replaces SnakeGymEnv.reset() (SnakeGymEnv.py:28-31 -> snake.py:96-99,119-127) for every
 * env whose mask byte is non-zero (mask == NULL: all).  obs_dev [n_envs x obs_dim] f32,
 * device pointer; rows of unmasked envs are left untouched.  stream = hipStream_t or NULL.
 * The env lands on ITS row of the reset-pose table (snk_set_reset_pose below; after snk_create: zeros and the unit
 * quaternion), with zero base twist and joint velocities; the reward's previous x becomes the pose's x. */
int snk_reset(snk_handle* h, const uint8_t* mask_dev, float* obs_dev, void* stream);

/* Replaces SubprocVecEnv.step (ppo/multiprocessing_env.py:119-128) = per env
 * SnakeGymEnv.step (SnakeGymEnv.py:33-50) -> Snake.step (snake.py:274-306) with its
 * 0..41 stepSimulation calls, reward, termination, -5 and auto-reset.
 *   actions_dev  [n_envs x act_dim] f32, device; clipped to [-1,1] IN PLACE like
 *                checkBound (SnakeGymEnv.py:82-88)
 *   obs_dev      [n_envs x obs_dim] f32   rew_dev [n_envs] f32   done_dev [n_envs] u8
 *   substeps_dev [n_envs] i32 (may be NULL): Snake.counter
 *   vec_mode     1: worker semantics, obs of a done env is the post-reset one
 *                (multiprocessing_env.py:13-15); 0: SnakeGymEnv.step semantics, terminal obs
 * Asynchronous on `stream`; results are ready after the stream is synchronised.
 * Internally two launches: a one-block plan kernel and the step kernel, whose resident waves share
 * the env-steps through an in-launch queue.  Results do not depend on that schedule.
 * Every wait inside the kernel is bounded; if one ever runs out the kernel drains, and this and
 * every later call on the handle return non-zero ("env-step scheduler: ...").  Environment:
 * SNK_QUANTUM=<substeps per slice> (default 1; 0 = the unscheduled kernel), SNK_FORCE_STREAMED=1 (16 links on the
 * streamed-row kernels of the 32-link chain: diagnostics and cross-checks), SNK_MOTORS_APART=1 (the register-resident
 * substep builds its motor rows in a batch of their own at every contact count: cross-checks), SNK_SUPPORT_SERIAL=1 (the
 * contact functions find a hull's support vertex with one load per candidate instead of in the lanes' copy of the vertex
 * table: cross-checks), all read by snk_create. */
int snk_step(snk_handle* h, float* actions_dev, float* obs_dev, float* rew_dev,
             uint8_t* done_dev, int32_t* substeps_dev, int32_t vec_mode, void* stream);

/* The reset-pose table: what Snake.initPosition, Snake.initOrientation and Snake.initState (snake.py:22-24) are to the
 * reference's soft reset -- resetPositionOrientation (snake.py:126-127) and resetPose (snake.py:119-124) read them at
 * every reset -- held per environment on the device, because the reset of a finished episode happens inside the step
 * kernel (SnakeGymEnv.py:39-41).  One row per env: [position 3 | orientation quaternion xyzw 4 | joint angles n].
 * snk_create fills the reference's defaults (zeros, quaternion 0 0 0 1); the state right after snk_create is the zero
 * pose whatever is set later (the hard reset loads the snake at [0,0,0]: snake.py:93).  snk_reset and the auto-reset of
 * snk_step / snk_step_packed / snk_step_traced put an env on its row: pose as given, base twist zero
 * (resetBasePositionAndOrientation [U]), q = the row's angles, qd = 0 (resetJointState); motor torques, the joint-0
 * force, the contact cache and a free box persist.  The reward's previous x (SnakeGymEnv.py:30, 91) becomes the row's x
 * after snk_reset and after a vec_mode 1 auto-reset; vec_mode 0 keeps the terminal x (SnakeGymEnv.py:41-42).
 *
 * snk_reset_pose_floats (replaces len(initPosition) + len(initOrientation) + len(initState), snake.py:22-24): 7 + n, the
 * length of a caller-side row (the device rows are padded to whole 128-byte lines; callers never see that).
 *
 * snk_set_reset_pose (replaces assigning robot.initPosition / initOrientation / initState, snake.py:22-24): host
 * buffers; mask [n_envs] bytes (NULL: all), pose [n_envs x (7 + n)].  Synchronises the device first, like the state
 * accessors.  Rows of unmasked envs are neither read nor written.  Refused, with the env and the field named, and with
 * nothing written: a non-finite value; a quaternion whose norm differs from 1 by more than 1e-3.  The quaternion is
 * stored as given, not normalised.  Joint angles outside [joint_lo, joint_hi] are accepted: resetJointState does not
 * clamp, and the limit rows act on the next substep.
 *
 * snk_get_reset_pose (replaces reading the three attributes back, snake.py:22-24): host buffer [n_envs x (7 + n)].
 *
 * snk_set_reset_pose_dev (replaces the same assignment, snake.py:22-24, for a trainer whose data never leaves the GPU):
 * mask_dev [n_envs] bytes (NULL: all) and pose_dev [n_envs x (7 + n)] f32 are DEVICE pointers; a small copy kernel,
 * asynchronous on `stream` (hipStream_t or NULL) and therefore ordered with the steps and resets enqueued there -- e.g. new
 * poses for exactly the envs whose done flag the last step set, before the next step, without touching the host.  The
 * values cannot be validated here: a non-finite value or a non-unit quaternion goes into the table as it is, and into
 * the env's state at its next reset.
 *
 * All four refuse a null handle and a poisoned one (snk_debug_raise_alarm) with snk_last_error() set:
 * snk_reset_pose_floats by returning 0, the others by returning non-zero. */
int32_t snk_reset_pose_floats(const snk_handle* h);
int snk_set_reset_pose(snk_handle* h, const uint8_t* mask /* host, NULL: all */, const float* pose /* host [n_envs x (7+n)] */);
int snk_get_reset_pose(snk_handle* h, float* pose /* host [n_envs x (7+n)] */);
int snk_set_reset_pose_dev(snk_handle* h, const uint8_t* mask_dev, const float* pose_dev, void* stream);

/* The same step with ONE output buffer: packed_dev [n_envs x row_stride] f32 (row_stride >= obs_dim + 2), row e =
 * [obs of env e (obs_dim floats) | reward (f32) | done (u32: 0 or 1) | untouched padding].  This is the block a rank of a
 * sharded vector env sends to the trainer rank -- the reference's workers send (ob, reward, done, info) per env through
 * their Pipe (ppo/multiprocessing_env.py:11-16, 125-128) -- written by the step kernel itself, so that no copy kernel
 * stands between the physics and the gather (bullet-envs_amd/device_env.py: ShardedVecEnv). */
int snk_step_packed(snk_handle* h, float* actions_dev, float* packed_dev, int32_t row_stride,
                    int32_t* substeps_dev, int32_t vec_mode, void* stream);

/* Test-mode telemetry, written by the step kernel itself.  Replaces what Snake.step collects in mode 'test' after
 * every stepSimulation of its servo loop (snake.py:275-293: step_internal_observations.append(getObservation()),
 * link_positions.append(getLinkPositions())) and SnakeGymEnv.step hands out as info['internal_observations'] /
 * info['link_positions'] (SnakeGymEnv.py:43-44; ppo/test.py:84-105 concatenates them into the saved trajectories).
 *
 * snk_trace_row_floats: floats per trace row = the payload, 3n + 8 observation floats + 3(n + 1) link-position floats,
 * rounded up to a multiple of 32 floats (whole 128-byte lines): 107 -> 128 for 16 links, 203 -> 224 for 32 links.
 *
 * snk_step_traced: snk_step (same contract, same results bit for bit) that also writes, after physics substep s of env
 * e's env-step, row s of that env:
 *   trace_dev [n_envs x trace_rows x snk_trace_row_floats] f32, device, 128-byte aligned;
 *   row = [ getObservation after the substep (3n + 8) | getLinkPositions x_0..x_n, y_0..y_n, z_0..z_n | padding ].
 * Rows s >= substeps_dev[e] and every row's padding are never touched; an env-step of 0 substeps writes nothing.  The
 * rows of an env whose episode ended in this step hold that step (pre-reset state: the reference clears its lists at the
 * start of the next step, snake.py:276-278, not in reset).  Every row's joint-0 force and motor torques are its own
 * substep's (the kernel evaluates the sensor pass on every substep of a traced step; snk_step only where it can be
 * observed).  substeps_dev is required; trace_rows >= max_counter + 1, else the call refuses.  A misaligned trace_dev is
 * refused. */
int32_t snk_trace_row_floats(const snk_handle* h);
int snk_step_traced(snk_handle* h, float* actions_dev, float* obs_dev, float* rew_dev, uint8_t* done_dev,
                    int32_t* substeps_dev, float* trace_dev, int32_t trace_rows, int32_t vec_mode, void* stream);

/* Host-buffer convenience forms (upload, run, download, synchronise). */
int snk_reset_host(snk_handle* h, const uint8_t* mask, float* obs);
int snk_step_host(snk_handle* h, float* actions, float* obs, float* rew, uint8_t* done,
                  int32_t* substeps, int32_t vec_mode);
/* snk_step_traced with host buffers; trace [n_envs x trace_rows x snk_trace_row_floats] f32.  The device trace buffer
 * belongs to the handle (allocated on the first call, again when trace_rows changes).  What the kernel does not write
 * (padding, rows >= substeps[e]) comes back as NaN (all bits set), whatever `trace` held before. */
int snk_step_traced_host(snk_handle* h, float* actions, float* obs, float* rew, uint8_t* done, int32_t* substeps,
                         float* trace, int32_t trace_rows, int32_t vec_mode);

/* Replaces pybullet.stepSimulation (snake.py:286) preceded by setJointMotorControlArray
 * (snake.py:221): k physics substeps with motor targets [n_envs x n] (radians), host buffer.
 * info (may be NULL) [n_envs x 2] i32: solver iterations and contact count of the last substep.
 * For single-substep parity tests. */
int snk_substep_host(snk_handle* h, const float* targets, int32_t k, int32_t* info);

/* ---------------------------------------------------------------------------------------------------------------------
 * The tensor seam: the physics below the fused env-step, driven from device memory.  With these calls the loop of
 * Snake.step (snake.py:283-304) -- or any other reward, termination, gait or control rate -- can be written by the
 * caller on device tensors, one launch per call, nothing touching the host.  Every device-pointer form is asynchronous
 * on `stream` (hipStream_t or NULL) and ordered with the steps, resets and renders enqueued there; none synchronises,
 * copies or validates what lies in device memory.
 *
 * snk_substep (replaces pybullet.stepSimulation, snake.py:286, behind setJointMotorControlArray, snake.py:219-221): k
 * physics substeps towards targets_dev [n_envs x n] f32 (radians).  It is snk_substep_host without the copies and the
 * synchronisation, plus a mask: active_dev [n_envs] u8 or NULL (all).  An env whose byte is 0 is neither loaded nor
 * stored: its record, contact cache, free box and info row keep their bits.  info_dev [n_envs x 2] i32 or NULL: solver
 * iterations and contact count of the last substep.  The sensor pass runs on every substep, as in snk_substep_host.
 *
 * snk_observe (replaces Snake.getObservation snake.py:209-217, checkSnakeHeight's mean z snake.py:237-245 and
 * Snake.getLinkPositions snake.py:138-146 in one pass): obs_dev [n_envs x obs_dim], height_dev [n_envs], linkpos_dev
 * [n_envs x 3(n+1)] laid out as snk_link_positions; each may be NULL, all three NULL is refused. */
int snk_substep(snk_handle* h, const float* targets_dev, int32_t k, const uint8_t* active_dev, int32_t* info_dev, void* stream);
int snk_observe(snk_handle* h, float* obs_dev, float* height_dev, float* linkpos_dev, void* stream);

/* snk_link_states (replaces pybullet.getLinkState(computeLinkVelocity=1) over every link, and getBasePositionAndOrientation
 * / getBaseVelocity for the root: what Snake.getLinkPositions and Snake.getLinkOrientations, snake.py:138-156, read link
 * by link) for any subset of the handle's envs at once, from their CURRENT device state.
 *   snk_link_state_rows  3n + 2: the links of the unmerged URDF tree.  Row r is Bullet link r - 1: row 0 the root
 *                (kdl_dummy_root, Bullet's base, link -1), row 1 `base`, rows 3k - 1, 3k, 3k + 1 INPUT_IF_k, COLLAR_k and
 *                OUTPUT_BODY_k -- row i + 1 is the link of joint i.  0 (snk_last_error set) for a null handle.
 *   env_ids_dev  [n_rows] i32, device; NULL: envs 0 .. n_rows - 1.  snk_render's rule: ids may repeat and come in any
 *                order; they cannot be validated on this path, an id outside 0 .. n_envs - 1 reads nothing and its rows
 *                are written as zeros.
 *   out_dev      [n_rows][3n + 2][16] f32, 16-byte aligned.  A row:
 *                  0-2 COM world position | 3-6 world orientation, quaternion xyzw | 7-9 world origin of the URDF link
 *                  frame | 10-12 world linear velocity of the COM | 13-15 world angular velocity
 *                -- PyBullet's getLinkState tuple without its two constant entries (snk_link_inertial_offsets has the
 *                first; the second is the identity: the model's inertias are diagonal in link axes, so the inertial frame
 *                is axis-parallel to the link frame and the one quaternion serves both orientations).
 * Row 0 carries the record's own position, quaternion, omega and velocity verbatim: bitwise what snk_get_state returns.
 * The other rows take their quaternion from the link's rotation matrix by the branch of the largest of (trace, m00,
 * m11, m22) (Shepperd), normalised and signed so that w >= 0.  The COM velocity is v(body origin) + omega x (COM - body
 * origin), the joint's own rate being part of the body's twist.  Bytes beyond [n_rows][3n + 2][16] are left alone;
 * nothing of the handle's state is written.  Refused, naming the argument: a null or poisoned handle; n_rows < 1; a null
 * or misaligned out_dev.
 *
 * snk_link_states_host: the same with HOST buffers (replaces the same getLinkState loop for a caller on the host); it
 * synchronises the device first, like the state accessors, and also refuses an env id outside 0 .. n_envs - 1 and n_rows
 * above n_envs without ids, each with its index.
 *
 * snk_link_inertial_offsets (replaces getLinkState(...)[2] and getDynamicsInfo(...)[3], localInertialFramePosition):
 * host only, no handle and no device.  out [(3n+2) x 3]: every link's COM in its own link frame, from the same sub-link
 * offsets the model compiler merges into the composite bodies. */
int32_t snk_link_state_rows(const snk_handle* h);
int snk_link_states(snk_handle* h, const int32_t* env_ids_dev, int32_t n_rows, float* out_dev, void* stream);
int snk_link_states_host(snk_handle* h, const int32_t* env_ids, int32_t n_rows, float* out);
int snk_link_inertial_offsets(const snk_params* p, double* out);

/* snk_copy_envs (replaces pybullet.saveState in one world + restoreState in another, which the reference never needs --
 * snake.py:96-99 resets instead -- and a sampling-based controller does: forking env states): env dst[i] becomes env
 * src[i] in everything that is simulator state -- the whole state record (state, aux, joint-3 force, previous x), the
 * link manifolds (contact_model 1), the free box and its manifold (obstacle 2), the ground friction; with
 * SNK_COPY_RESET_POSE in flags the env's row of the reset-pose table as well.  src_ids_dev, dst_ids_dev [n_pairs] i32,
 * device.  One workgroup per pair copies whole table rows, padding included.
 * THE CONTRACT, which cannot be validated on this path (the limit snk_set_reset_pose_dev has): the dst ids are distinct,
 * and no id is both a source and a destination -- otherwise which copy wins is undefined, and nothing worse happens.  A
 * pair with an id outside 0 .. n_envs - 1 is a no-op.  Refused: a null or poisoned handle, a null id list, n_pairs < 1,
 * unknown bits in flags.
 * snk_copy_envs_host: the same with HOST id lists (synchronises first); it does validate: an id outside the handle, a
 * repeated dst, or a dst that is also a src is refused, naming the index, with nothing written.
 * ------------------------------------------------------------------------------------------------------------------- */
#define SNK_COPY_RESET_POSE 1   /* flags bit: copy the reset-pose row too */
int snk_copy_envs(snk_handle* h, const int32_t* src_ids_dev, const int32_t* dst_ids_dev, int32_t n_pairs, int32_t flags,
                  void* stream);
int snk_copy_envs_host(snk_handle* h, const int32_t* src_ids, const int32_t* dst_ids, int32_t n_pairs, int32_t flags);

/* ---------------------------------------------------------------------------------------------------------------------
 * The reported contacts: the contract of snk_contacts (replaces pybullet.getContactPoints(snake, plane) and
 * getContactPoints(block, plane), which the reference never calls and a reward written over the tensor seam does: touch
 * flags, ground-reaction terms).  The kernel (bullet-envs_amd/csrc/snk_world.hpp: contacts_kernel) and the independent
 * numpy model of the tests (tests/np_contacts.py) are both written from this text.  contact_model 1 only: what is
 * reported is the contact CACHE the handle holds (snk_get_manifold, snk_get_box), read where it lies.
 *
 * Contact slots.  One env's contacts are a fixed table of slots.  snk_contact_slots(h) = 4 * 2n, and 4 * 2n + 4 on an
 * obstacle 2 handle; 0, with snk_last_error set, for a contact_model 0 handle, a null handle or a poisoned one (the calls
 * below then refuse).  Slot 4 c + j is cached point j of cylinder c, the cylinders in link order: the order of
 * snk_get_manifold.  The last four slots of an obstacle 2 handle are the free box's points with the plane.
 *
 * The record.  A slot is 16 floats:
 *   0-2    the point on the moving body in world coordinates at the CURRENT pose.  Cylinder c, cached point a (in its
 *          link's coordinates): centre_c + Rw_c (a - (0, 0, cyl_zoff)), centre_c and Rw_c the cylinder's world frame as the
 *          contact finder's refresh forms it -- Rw_c = R_b cyl_R[c], centre_c = o_b + R_b cyl_c[c] on the frame (R_b, o_b)
 *          of composite body b = (c + 1) / 2 from the forward kinematics; cyl_zoff as snk_params_derived reports it.
 *          The box: pos + R(quat) a, pos and quat as snk_get_box reports them.
 *   3-5    the point on the ground as cached: (b.x, b.y, 0).
 *   6-8    the contact normal on the ground, towards the body: (0, 0, 1).
 *   9      the distance at the current pose: float 2 - float 5.  (The cached point already contains the collision margin.)
 *   10     the normal force in newtons: the cached impulse / dt, dt the handle's time step as the kernels hold it (float32).
 *   11     the cached impulse itself.
 *   12     the cylinder index c; 2n for the box.  (Small integers: exact as floats.)
 *   13     j.
 *   14     1.0 if the slot is live (j < the cylinder's count, the count taken as 0 .. 4), else 0.0.
 *   15     0.
 * A slot that is not live is sixteen zeros, whatever stale point the cache keeps there.
 *
 * What the numbers mean.
 *   - The positions are those of the pose the state holds NOW.  PyBullet's getContactPoints reports them as of the last
 *     collision pass, one dt of motion earlier; the cache does not keep that pass's distances: a documented deviation
 *     (DESIGN.md 3).
 *   - The force is that of the last substep in which the point had a row.  An env-step of 0 substeps leaves it stale.
 *   - A cached point that the next refresh would drop (beyond the breaking threshold at the current pose) is reported
 *     as the cache holds it.  The cache is the state.
 *   - Link-link and link-box contacts are stateless in the kernels and carry no stored impulse: they are NOT reported
 *     (their geometry is what snk_closest_points computes, below).  Friction impulses are not stored either.
 *
 * Outputs, per requested env (row):
 *   points_dev  [n_rows][slots][16] f32, 16-byte aligned;
 *   force_dev   [n_rows][2n + 1] f32: per cylinder the sum of float 10 over its live slots, j ascending; entry 2n is the
 *               box's, 0 without obstacle 2;
 *   count_dev   [n_rows] i32: the number of live slots.
 * Each may be NULL; all three NULL is refused.
 *
 * snk_contacts follows snk_link_states' shape and rules: env_ids_dev [n_rows] i32 or NULL (envs 0 .. n_rows - 1), ids may
 * repeat and come in any order; an id outside 0 .. n_envs - 1 reads nothing and its outputs are zeros.  Asynchronous on
 * `stream`, one launch (one wave per row), no atomics and no waits; it does not synchronise, copy or validate.  Bytes
 * beyond the outputs are left alone; nothing of the handle's state is written, nothing is allocated.  Refused, naming the
 * argument: a null or poisoned handle; a contact_model 0 handle; n_rows < 1; all three outputs null; a misaligned
 * points_dev.
 * snk_contacts_host: the same with HOST buffers; it synchronises the device first, like the state accessors, and also
 * refuses an env id outside 0 .. n_envs - 1 and n_rows above n_envs without ids, each with its index.
 * snk_contact_links: host only, no handle and no device.  out [2n] i32: the Bullet link index of every cylinder's link
 * (INPUT_INTERFACE_k = 3k - 2 for even c = 2k - 2, OUTPUT_BODY_k = 3k for odd c = 2k - 1) -- PyBullet's linkIndexA, and
 * row link + 1 of snk_link_states.
 * ------------------------------------------------------------------------------------------------------------------- */
#define SNK_CONTACT_FLOATS 16   /* floats per contact slot */
int32_t snk_contact_slots(const snk_handle* h);
int snk_contacts(snk_handle* h, const int32_t* env_ids_dev, int32_t n_rows, float* points_dev, float* force_dev,
                 int32_t* count_dev, void* stream);
int snk_contacts_host(snk_handle* h, const int32_t* env_ids, int32_t n_rows, float* points, float* force, int32_t* count);
int snk_contact_links(const snk_params* p, int32_t* out /* [2n] */);

/* ---------------------------------------------------------------------------------------------------------------------
 * The closest points: the contract of snk_closest_points (replaces pybullet.getClosestPoints(snake, block, distance) and
 * getClosestPoints(snake, snake, distance): "how far is each link from the block", "is the snake folding onto itself" --
 * the obstacle is the only other body the reference simulates, snake_gait_test.py:51).  The kernel
 * (bullet-envs_amd/csrc/snk_world.hpp: closest_points_kernel) and the tests (tests/np_closest.py) are both written from
 * this text.  It is the solver's narrow phase (csrc/snk_selfcol.hpp) run as a query: at a caller-given distance, for any
 * subset of envs, writing tensors and touching no state.
 *
 * The query.  Geometry of the pose the state holds NOW, the pose snk_link_states reports.  `distance` (metres, finite,
 * >= 0) is PyBullet's argument: a pair is FOUND when its distance is < distance (strict, as the solver's test against its
 * breaking threshold), the distance taken between the margin-inflated shapes: the GJK distance of the cores less both
 * collision margins.  At distance = snk_params_derived(...)[0], the handle's own breaking threshold, the found pairs are
 * exactly the link-link and link-box contacts the next substep's streamed-row solve would build rows for; above it the
 * call is a proximity sensor.  (hull_sides 0: the implicit cylinder's GJK runs on here to a relative duality gap of 1e-6,
 * the solver's stops at 1e-5 -- its distances are good to 1e-7 m, its normals to 3e-3 rad only --, so a pair within 1e-7 m
 * of the threshold may be found by one and not by the other.)  The link-link part is computed whatever self_collision says: it is a geometry query.  The
 * box is the static one (obstacle 1: obstacle_pos, identity rotation) or the free one where it is now (obstacle 2: centre
 * and quaternion as snk_get_box reports them, R(quat) formed as snk_contacts forms it).  On a handle without an obstacle
 * the box part is empty, not refused.
 *
 * The narrow phase, for a cylinder A and B = the box or a cylinder b > a.  Tier 0: GJK on the core shapes (the 32-gon hull
 * or the implicit cylinder, as hull_sides says; the box's core is smaller than the nominal box by the margin), margin mg =
 * collision_margin.  Tier 1, when those cores overlap: GJK on cores shrunk by 6 mm, mg = collision_margin + 6 mm.  With
 * witness points pa, pb at core distance d: normal n = (pa - pb) / d, distance d - 2 mg, and the reported points lie on the
 * inflated surfaces: P = pa - n mg on A, PB = pb + n mg on B.  Tier 2, when the shrunk cores overlap too: the line of
 * centres -- n = (c_A - c_B) / |c_A - c_B| (for coincident centres (0, 0, 1), against the box (-1, 0, 0)), distance
 * -2 (collision_margin + 6 mm), P = PB = the midpoint of the centres, against the box the cylinder's centre.  The broad
 * phase (bounding spheres) and the separating-axis culls in front of it take `distance` and are conservative: a culled
 * pair is one the narrow phase would reject.  One point per pair (PyBullet reports up to four per pair, from its cache).
 *
 * Slots.  One env's table has snk_closest_slots(h, max_pairs) = 2n + max_pairs slots of SNK_CONTACT_FLOATS floats.
 *   slots 0 .. 2n - 1   slot c is the pair (cylinder c, box): dense; live only if found and flags has SNK_PAIRS_BOX.
 *   slots 2n ..         the found link-link pairs, compact, in the solver's order: by offset b - a = 2, 3, ..., then by a
 *                       (consecutive cylinders, b - a = 1, are parent and child and are no pair).  When more than
 *                       max_pairs are found, the first max_pairs in that order are written.
 * max_pairs is in 0 .. snk_link_pairs(h) = C(2n, 2) - (2n - 1): 465 for 16 links, 1953 for 32.
 * The record:
 *   0-2    the point on A = cylinder a, world coordinates, on the inflated surface
 *   3-5    the point on B (the box, or cylinder b > a)
 *   6-8    the unit normal on B, towards A (link-box: from the box to the link, as the solver has it)
 *   9      the distance (negative: penetration); float 0-2 less float 3-5 is float 6-8 times it
 *   10     the tier: 0, 1 or 2
 *   11     0 (no force: these contacts carry no stored impulse)
 *   12     a
 *   13     b; 2n for the box.  (Small integers: exact as floats.)
 *   14     1.0 if the slot is live
 *   15     0.
 * A slot that is not live is sixteen zeros.
 *
 * Outputs, per requested env (row):
 *   points_dev     [n_rows][2n + max_pairs][16] f32, 16-byte aligned;
 *   clearance_dev  [n_rows][2][2n] f32: row 0 per cylinder its distance to the box, row 1 per cylinder the least distance
 *                  over the link-link pairs it belongs to -- each min(found distances, distance), so that `distance` reads
 *                  "nothing within reach".  Row 1 counts every found pair, those beyond max_pairs included; a part not
 *                  asked for in flags is filled with `distance`;
 *   count_dev      [n_rows][2] i32: box pairs found, link-link pairs found -- the second NOT clipped to max_pairs, so that
 *                  truncation shows.
 * Each may be NULL; all three NULL is refused.
 *
 * snk_closest_points follows snk_contacts' shape and rules: env_ids_dev [n_rows] i32 or NULL (envs 0 .. n_rows - 1), ids may
 * repeat and come in any order; an id outside 0 .. n_envs - 1 reads nothing and ALL its outputs are zeros (its clearance
 * too).  Asynchronous on `stream`, one launch (one wave per row), no atomics to memory and no waits; it does not
 * synchronise, copy or allocate.  Bytes beyond the outputs are left alone; nothing of the handle's state is written.
 * Refused, naming the argument: a null or poisoned handle; n_rows < 1; a non-finite or negative distance; zero or unknown
 * bits in flags; all three outputs null; a misaligned points_dev; max_pairs outside 0 .. snk_link_pairs(h).
 * snk_closest_points_host: the same with HOST buffers; it synchronises the device first, like the state accessors, and also
 * refuses an env id outside 0 .. n_envs - 1 and n_rows above n_envs without ids, each with its index.
 * snk_link_pairs, snk_closest_slots: 0, with snk_last_error set, for a null or poisoned handle (snk_closest_slots also for a
 * max_pairs out of range).
 * ------------------------------------------------------------------------------------------------------------------- */
#define SNK_PAIRS_BOX   1   /* flags: the 2n (cylinder, obstacle box) pairs */
#define SNK_PAIRS_LINKS 2   /* flags: the link-link pairs (every cylinder pair except consecutive cylinders) */
int32_t snk_link_pairs(const snk_handle* h);
int32_t snk_closest_slots(const snk_handle* h, int32_t max_pairs);
int snk_closest_points(snk_handle* h, const int32_t* env_ids_dev, int32_t n_rows, float distance, int32_t flags,
                       int32_t max_pairs, float* points_dev, float* clearance_dev, int32_t* count_dev, void* stream);
int snk_closest_points_host(snk_handle* h, const int32_t* env_ids, int32_t n_rows, float distance, int32_t flags,
                            int32_t max_pairs, float* points, float* clearance, int32_t* count);

/* State access (host buffers), for parity tests and checkpointing.  These calls (and snk_get_obs,
 * snk_mean_height, snk_link_positions, snk_set/get_ground_friction) synchronise the device first, so a step
 * still running on any stream is complete before the records are read or overwritten.
 * state [n_envs x state_dim]; aux [n_envs x (n+2)] = motor torques n, joint-0 Fz, prev obs x. */
int snk_get_state(snk_handle* h, float* state, float* aux);
int snk_set_state(snk_handle* h, const float* state, const float* aux);
/* contact_model 1 only: the persistent contact manifolds (part of the simulator state, like Bullet's contact cache,
 * which a soft reset does not clear [U]).  Host buffers [n_envs x 2n x 29]: per cylinder (in link order)
 * [count, 4 x (point on the link in link coordinates 3, point on the ground in world coordinates 3, the normal impulse
 * the point carried in the last substep)].
 * snk_manifold_floats = 2n * 29, or 0 for a contact_model 0 handle or a null handle (then get/set fail). */
int32_t snk_manifold_floats(const snk_handle* h);
int snk_get_manifold(snk_handle* h, float* out);
int snk_set_manifold(snk_handle* h, const float* in);
/* getObservation (snake.py:209-217) of every env, host buffer [n_envs x obs_dim]. */
int snk_get_obs(snk_handle* h, float* obs);
/* checkSnakeHeight's mean z (snake.py:237-245), host buffer [n_envs]. */
int snk_mean_height(snk_handle* h, float* out);
/* Snake.getLinkPositions (snake.py:138-146), the test-mode telemetry of SnakeGymEnv.step's info
 * (SnakeGymEnv.py:43-44): world COM of Bullet links 0,3,...,3n of every env, host buffer
 * [n_envs x 3(n+1)] laid out [x_0..x_n, y_0..y_n, z_0..z_n]. */
int snk_link_positions(snk_handle* h, float* out);

/* Reaction force through the first motor joint (Bullet joint 3: INPUT_IF_1 -> OUTPUT_BODY_1), z component in the
 * child link's frame, of every env's last physics substep: what snake_gait_test.py:33-40,126 reads
 * (getJointState(robot, 3)[2][2], "> 20: the snake has hit the wall").  Host buffer [n_envs].  Like the joint-0 force
 * of the observation it is evaluated on the last substep of an env-step (and by every snk_substep_host substep). */
int snk_joint3_reaction_fz(snk_handle* h, float* out);

/* obstacle 2 only: the free box of every env (part of the simulator state; a soft reset leaves it where it is, like
 * resetBasePositionAndOrientation of the SNAKE, snake.py:126-127).  Host buffers: state [n_envs x 13] = pos3,
 * quat xyzw 4, omega_world 3, vel_world 3; manifold [n_envs x 29] = its contact cache with the plane, [count, 4 x
 * (point on the box in box coordinates 3, point on the ground 3, applied normal impulse)].  Either may be NULL. */
int snk_get_box(snk_handle* h, float* state, float* manifold);
int snk_set_box(snk_handle* h, const float* state, const float* manifold);

/* ---------------------------------------------------------------------------------------------------------------------
 * The rendered scene: the contract of snk_render.  The kernels (bullet-envs_amd/csrc/snk_render.hpp) and the independent
 * float64 model of the tests (tests/np_render.py) are both written from this text.
 *
 * Camera.  A camera is 32 floats: the view matrix V, then the projection matrix P, each column-major 4x4 with the OpenGL
 * clip convention, as PyBullet passes them.  M = P V; its inverse is taken in float64 and rounded to float32.  Pixel
 * (row j from the top, column i) of a width x height image is sampled at its centre: x = 2 (i + 0.5) / width - 1,
 * y = 1 - 2 (j + 0.5) / height.  a = M^-1 (x, y, -1, 1) and b = M^-1 (x, y, +1, 1) are the pixel centre on the near and on
 * the far plane; o = a.xyz / a.w, f = b.xyz / b.w.  The ray is o + t d with d = (f - o) / |f - o|, t in metres, and only
 * hits with 0 <= t <= |f - o| count: those between the near and the far plane, i.e. with a depth in [0, 1].
 *
 * Solids are convex and drawn one-sided: a ray meets a solid where it ENTERS it.  A solid the ray starts inside of (one
 * the near plane cuts) is open along that ray: what lies behind it shows.
 *   ground    the plane z = 0, normal +z, primitive id 0.  It carries a 0.5 m checkerboard: a hit at (x, y) has parity
 *             (floor(x / 0.5) + floor(y / 0.5)) & 1; albedo (0.95, 0.95, 0.95) for parity 0, (0.55, 0.65, 0.85) for 1.
 *   cylinder  c = 0 .. 2n - 1, primitive id 1 + c: the link colliders (the model's cyl_body / cyl_c / cyl_R on the body
 *             frames of the forward kinematics; radius and half length as snk_params_derived reports them), finite and
 *             capped: the points within the radius of the axis and within the half length of the centre along it.  The
 *             normal is radial where the ray enters through the side, +-axis where it enters through a cap.  Albedo
 *             (0.85, 0.35, 0.15) for even c, (0.25, 0.25, 0.28) for odd c.
 *   box       primitive id 1 + 2n.  obstacle 1: centre obstacle_pos, half extents obstacle_half, axis aligned;
 *             obstacle 2: the env's free box (centre and quaternion as snk_get_box reports them); obstacle 0: none.
 *             The normal is that of the face (slab) the ray enters through.  Albedo (0.45, 0.75, 0.45).
 * The hit drawn is the nearest; the primitives are tried in the order of their ids, and a later one replaces the kept hit
 * only when its t is smaller by more than 2e-4 m.  (Two consecutive colliders of one body are coaxial, of one radius, and
 * overlap by 5.7 mm along the axis -- snake.urdf:806-811, 862-867, 877 -- so their side surfaces coincide there: without
 * the margin, round-off would pick the colour: the float32 twin of tests/np_render.py moved t by 3e-5 m at one such pixel
 * near a silhouette.  The lower id is drawn.  The margin holds between ANY two primitives, the ground included: a solid
 * less than 0.2 mm in front of an earlier one loses to it.)
 * No hit: RGBA (200, 215, 235, 255), depth 1.0, segmentation -1.
 *
 * Shading.  colour = albedo x (0.4 + 0.6 x max(0, n.L) x lit), n the outward normal at the hit, L = (0.4, -0.3, 0.85)
 * normalised.  lit = 1 without SNK_RENDER_SHADOW.  With it: lit = 0 where n.L <= 0 (the colour is the same either way),
 * else lit = 0 when the ray from the hit point moved 1e-4 m along n, towards L, meets a cylinder or the box at any
 * t >= 0 (a ray that starts inside one counts as meeting it), else 1.  Channel = (uint8) floor(255 c + 0.5); alpha 255.
 * Depth = 0.5 (M X).z / (M X).w + 0.5 at the hit point X: the OpenGL depth-buffer value getCameraImage returns, which
 * PyBullet's documented far near / (far - (far - near) depth) turns back into a distance along the view axis.
 *
 * Deviations from what PyBullet draws: it draws the STL visual meshes, this the collision geometry; the
 * cylinder is the implicit one, at most r (1 - cos(pi / 32)) = 0.125 mm outside the 32-gon hull the physics uses; links
 * without a collision shape are not drawn; no anti-aliasing, textures or specular term.
 * ------------------------------------------------------------------------------------------------------------------- */
#define SNK_RENDER_SHADOW 1     /* flags bit: cast the shadow ray */

/* Replaces Snake.render (snake.py:308-334: resetDebugVisualizerCamera + getCameraImage, the frame SnakeGymEnv.render
 * hands out in test mode, SnakeGymEnv.py:52-58, and ppo/test.py:77 collects) and the getCameraImage of
 * snake_gait_test.py:19-26,112 -- for any subset of the handle's envs at once, from their CURRENT device state.
 *   env_ids_dev  [n_images] i32, device; NULL: envs 0 .. n_images - 1.  Ids may repeat and come in any order.  They
 *                cannot be validated from the host on this path (as snk_set_reset_pose_dev's values cannot): an id
 *                outside 0 .. n_envs - 1 reads nothing, and its image shows the ground alone.
 *   cameras_dev  [n_images][32] f32, or [1][32] when shared_camera != 0: view, then projection (above).  Not validated:
 *                a singular or non-finite camera gives an image of background and undefined depths, nothing worse.
 *   flags        0 or SNK_RENDER_SHADOW.
 *   rgba_dev     [n_images][height][width] u8 x 4 (4-byte aligned: a pixel is one 32-bit store);
 *   depth_dev    [n_images][height][width] f32, may be NULL;   seg_dev  the same in i32, may be NULL: the primitive id.
 * Asynchronous on `stream` (hipStream_t or NULL) and ordered with the steps enqueued there: a render behind a step
 * shows the state after it.  Two launches -- one wave per image builds the image's table of primitives (64 bytes each)
 * and its camera; one 256-thread workgroup per 16 x 16 pixel tile casts the rays -- with no atomics and no waits; every
 * byte outside [n_images][height][width] is left alone; nothing of the handle's state is written.  The tables live in
 * scratch memory of the handle, grown on demand -- the first call, and any call with more images than every call before,
 * frees and allocates, i.e. waits for the whole device once and must not happen while a stream is being captured into a
 * graph: render n_envs images once before capturing.  Like every call on a handle, renders are serialised by the caller.
 * Refused, naming the argument: a null or poisoned handle; n_images < 1; width or height outside 1 .. 4096; more than
 * 2^31 - 1 pixels in all; unknown bits in flags; a null (or misaligned) rgba_dev; a null cameras_dev. */
int snk_render(snk_handle* h, const int32_t* env_ids_dev, int32_t n_images, const float* cameras_dev, int32_t shared_camera,
               int32_t width, int32_t height, int32_t flags, uint8_t* rgba_dev, float* depth_dev, int32_t* seg_dev,
               void* stream);
/* The same (replaces snake.py:308-334 and snake_gait_test.py:19-26 for a caller on the host) with HOST buffers: it
 * synchronises the device first, like the state accessors, and also refuses an env id outside 0 .. n_envs - 1, n_images
 * above n_envs without ids, and a non-finite camera entry -- each with its index. */
int snk_render_host(snk_handle* h, const int32_t* env_ids, int32_t n_images, const float* cameras, int32_t shared_camera,
                    int32_t width, int32_t height, int32_t flags, uint8_t* rgba, float* depth, int32_t* seg);

/* Replaces pybullet.computeViewMatrixFromYawPitchRoll (snake.py:310-316) [U]: bullet3's b3ComputeViewMatrixFromYawPitchRoll
 * restated.  Host only, no handle.  The eye sits `distance` behind `target` along the forward axis (y for up_axis 2, z for
 * up_axis 1) turned by yaw about the up axis and pitch about x; the up vector is turned with it, so a pitch of -90
 * degrees (the reference's camera, snake.py:322-325) has no degenerate up vector.  roll_deg is accepted and NOT used:
 * bullet3 sets its roll to zero.  out: column-major 4x4.  up_axis other than 1 or 2 is refused. */
int snk_view_matrix_ypr(const float target[3], float distance, float yaw_deg, float pitch_deg, float roll_deg, int32_t up_axis,
                        float out[16]);
/* Replaces pybullet.computeProjectionMatrixFOV (snake.py:317-320) [U]: bullet3's b3ComputeProjectionMatrixFOV restated.
 * Host only, no handle.  out[0] = y / aspect, out[5] = y = 1 / tan(fov / 2), out[10] = (near + far) / (near - far),
 * out[11] = -1, out[14] = 2 far near / (near - far), the rest 0.  Nothing is refused: the reference's own call passes
 * farVal = nearVal (snake.py:320), and gets the infinite entries the formula gives. */
int snk_projection_fov(float fov_deg, float aspect, float near_val, float far_val, float out[16]);

/* ---------------------------------------------------------------------------------------------------------------------
 * The ray test: the contract of snk_ray_test (replaces pybullet.rayTest / rayTestBatch, with parentObjectUniqueId /
 * parentLinkIndex: a fan of rays that rides on a link -- a range sensor; the reference's only read-out of its block,
 * snake_gait_test.py:51, is indirect).  The kernels (bullet-envs_amd/csrc/snk_render.hpp) and the independent float64
 * model of the tests (tests/np_rays.py) are both written from this text.
 *
 * Rays.  A ray is 6 floats, [from 3 | to 3].  rays_dev is [n_rows][n_rays][6] f32 -- with SNK_RAYS_SHARED in flags ONE set
 * [n_rays][6] used for every row (a sensor's fixed fan) -- 4-byte aligned, nothing more: torch.cat((from, to), -1) works.
 * parent_row = -1: the rays are in world coordinates.  parent_row = 0 .. 3n + 1: they are in the frame of that row of
 * snk_link_states OF THE ROW'S OWN ENV, at the pose the state holds now: x_world = origin + R x, the origin the link's COM
 * (floats 0-2 of its row) and R the link's rotation (what floats 3-6 are the quaternion of; the kernel takes the matrix
 * from the forward kinematics, R(body) R(link in body), as snk_link_states forms it, not through the quaternion).  Row =
 * Bullet link + 1: PyBullet's parentLinkIndex L is row L + 1.  [U] PyBullet transforms attached rays by the link's cached
 * world transform, which is the inertial (COM) frame; snk_link_inertial_offsets turns that into the URDF link frame.
 * The ray is o + t d, o = from, d = (to - from) / |to - from|, t in metres; only hits with 0 <= t <= |to - from| count.
 *
 * What is hit.  The solids of "The rendered scene" above, verbatim, at the pose the state holds now -- the ground plane
 * z = 0 (met from either side, as there), the 2n capped implicit cylinders, the box of obstacle 1 / 2 -- each kind only
 * when its bit is set in flags (PyBullet's collisionFilterMask, per kind of body).  They are met where the ray ENTERS
 * them; a solid the ray starts inside of is open along that ray ([U] Bullet's convex cast reports no hit from inside
 * either).  The hit is the nearest; the primitives are tried in the order of their ids, and a later one replaces the kept
 * hit only when its t is smaller by more than 2e-4 m -- the render's tie rule, for the same coaxial 5.7 mm overlaps.
 * The render's deviation holds here too: the cylinder is the implicit one, at most r (1 - cos(pi / 32)) = 0.125 mm
 * outside the 32-gon hull the solver uses, so a range onto a link may be that much short.
 *
 * The record.  hits_dev is [n_rows][n_rays][8] f32, 16-byte aligned:
 *   0    the hit fraction t / |to - from| in [0, 1]: PyBullet's hitFraction
 *   1-3  the hit position, world coordinates, whatever frame the ray came in
 *   4-6  the outward unit normal at the hit, world coordinates: radial, or +-axis for a cap entry, or that of the entered
 *        face of the box, or (0, 0, 1) for the ground
 *   7    the primitive id as a float, as snk_render's segmentation: 0 ground, 1 + c cylinder c (snk_contact_links maps c
 *        to its Bullet link), 1 + 2n the box
 * A miss is [1, 0, 0, 0, 0, 0, 0, -1] (PyBullet: fraction 1, id -1, zero vectors).  Misses besides "nothing in the way":
 * a zero-length ray; a ray with a non-finite entry (or whose float32 length is not finite); every ray of a row whose env
 * id is outside 0 .. n_envs - 1, which reads nothing; flags selecting a kind the handle does not have (a box on obstacle
 * 0) -- not refused.  A zero record is never written: it would read as a hit on the ground at the ray's origin.
 *
 * The call.  Asynchronous on `stream` (hipStream_t or NULL) and ordered behind the steps enqueued there.  env_ids_dev
 * [n_rows] i32, device; NULL: envs 0 .. n_rows - 1; ids may repeat and come in any order.  Two launches -- one wave per
 * row builds the row's table of primitives and its parent frame; one 256-thread workgroup per (row, chunk of 256 rays)
 * casts them -- with no atomics and no waits; nothing of the handle's state is written; bytes beyond
 * [n_rows][n_rays][8] are left alone.  The tables live in the render's scratch memory of the handle, with exactly its
 * growth rule, rows counting as images: the first call, and any call with more rows than every render / ray call
 * before had images / rows, frees and allocates, i.e. waits for the whole device once and must not happen while a stream
 * is being captured into a graph: cast rays for n_envs rows once before capturing.
 * Refused, naming the argument: a null or poisoned handle; n_rows < 1; n_rays outside 1 .. 65536; more than 2^28 rays in
 * all; parent_row outside -1 .. 3n + 1; none of the three kind bits set, or unknown bits, in flags; a null (or
 * misaligned) rays_dev; a null or misaligned hits_dev.
 *
 * snk_ray_test_host: the same with HOST buffers; it synchronises the device first, like the state accessors, and also
 * refuses an env id outside 0 .. n_envs - 1, n_rows above n_envs without ids, and a non-finite ray entry -- each with its
 * index.
 * ------------------------------------------------------------------------------------------------------------------- */
#define SNK_RAY_FLOATS 6      /* a ray:  [from 3 | to 3] */
#define SNK_HIT_FLOATS 8      /* a hit:  [fraction | position 3 | normal 3 | primitive id] */
#define SNK_RAYS_GROUND 1     /* flags: what the rays can hit (PyBullet's collisionFilterMask, per kind of body) */
#define SNK_RAYS_SNAKE  2
#define SNK_RAYS_BOX    4
#define SNK_RAYS_SHARED 8     /* rays_dev is ONE set [n_rays][6] used for every row (a sensor's fixed fan) */
int snk_ray_test(snk_handle* h, const int32_t* env_ids_dev, int32_t n_rows, const float* rays_dev, int32_t n_rays,
                 int32_t parent_row, int32_t flags, float* hits_dev, void* stream);
int snk_ray_test_host(snk_handle* h, const int32_t* env_ids, int32_t n_rows, const float* rays, int32_t n_rays,
                      int32_t parent_row, int32_t flags, float* hits);

/* ---------------------------------------------------------------------------------------------------------------------
 * The dynamics queries: the contract of snk_dynamics and snk_jacobians (what PyBullet exposes as calculateMassMatrix,
 * calculateInverseDynamics(q, qd, 0) and calculateJacobian, which the reference never calls and gravity compensation,
 * operational-space control and momentum or energy terms of a reward written over the tensor seam do).  The kernels
 * (bullet-envs_amd/csrc/snk_dyn.hpp) and the independent numpy model of the tests (tests/np_dynamics.py) are both written
 * from this text.  Read-only: they report the rigid-body model at the pose and velocity the state holds NOW.
 *
 * Coordinates.  The generalised velocity is u = [omega_world 3 | v_world of the root link's origin 3 | qd n]: floats 7-9,
 * 10-12 and 13 + n .. 12 + 2n of snk_get_state, in the state's order.  nd = 6 + n components (22 for 16 links, 38 for 32):
 * snk_dyn_dofs(h); 0, with snk_last_error set, for a null or poisoned handle.  [U] PyBullet orders the base's six columns
 * in its own way (its floating-base forms of calculateMassMatrix and calculateJacobian are not read here): a caller who
 * compares with it permutes.  du/dt below is the plain time derivative of those components: for the base the CLASSICAL
 * acceleration of the root origin (d/dt of its world velocity), not the spatial one.
 *
 * snk_dynamics.  mass_dev [n_rows][nd][nd] f32, dense, 16-byte aligned (an env's block is whole 16-byte quads: 1936
 * bytes at 16 links, 5776 at 32): M(q) of the unmerged tree under the handle's inertia rules (inertia_from_file,
 * default_mass, collision_margin), so that 1/2 u^T M u is the kinetic energy.  Both triangles are written, from the same
 * arithmetic: M == M^T bit for bit.  bias_dev [n_rows][nd] f32, 4-byte aligned: h in  M du/dt + h = Q, Q the generalised
 * force of everything else (motors, contacts).  flags: SNK_BIAS_VELOCITY selects the Coriolis, centrifugal and gyroscopic
 * terms at the state's u; SNK_BIAS_GRAVITY adds minus the generalised gravity force, at the handle's gravity_z as the
 * kernels hold it (float32); gravity alone is calculateInverseDynamics(q, 0, 0).  With both bits h is computed in ONE
 * pass: it is not required to be, bit for bit, the sum of the two single-bit results.  h is rigid-body only: Bullet's
 * link damping, joint damping and the velocity clamp [U] are the integrator's business and are NOT in it (the step
 * kernels' per-body bias, body_bias in csrc/snk_dynamics.hpp, folds the damping terms in and is not this h).
 * Either output may be NULL; both NULL is refused.  A zero flags word and unknown bits are refused (also when only
 * mass_dev is asked for).
 *
 * snk_jacobians.  link_rows_dev [n_points] i32, device: rows of snk_link_states, 0 .. 3n + 1 (row = Bullet link + 1), ONE
 * list shared by every env row; n_points in 1 .. SNK_JAC_MAX_POINTS.  local_dev [n_points][3] f32 or NULL: the point in
 * the link's COM frame -- the frame of snk_ray_test's parent_row: origin the link's COM, axes the link's rotation; NULL:
 * the COM itself.  jac_dev [n_rows][n_points][6][nd] f32, 16-byte aligned: rows 0-2 the world linear velocity of the point
 * per unit of each component of u, rows 3-5 the link's world angular velocity, so that J u at the COM is floats 10-12 and
 * 13-15 of that link's row of snk_link_states.  The column of a joint that does not move the link is zeros, exactly; the
 * columns of v are the identity (rows 0-2) and zeros (rows 3-5), exactly.  A link row outside 0 .. 3n + 1 cannot be
 * refused on the device path: its Jacobian is written as zeros.
 *
 * Both follow snk_contacts' shape and rules: env_ids_dev [n_rows] i32 or NULL (envs 0 .. n_rows - 1), ids may repeat and
 * come in any order; an id outside 0 .. n_envs - 1 reads nothing and ALL its outputs are zeros.  Asynchronous on `stream`,
 * one launch (one wave per row), no atomics and no waits; they do not synchronise, copy or validate.  Bytes beyond the
 * outputs are left alone; nothing of the handle's state is written, nothing is allocated.  Refused, naming the argument:
 * a null or poisoned handle; n_rows < 1; bad flags; all outputs null; a misaligned mass_dev or jac_dev; n_points out of
 * range; a null link_rows_dev.
 * snk_dynamics_host / snk_jacobians_host: the same with HOST buffers; they synchronise the device first, like the state
 * accessors, and also refuse an env id outside 0 .. n_envs - 1, n_rows above n_envs without ids, a link row outside
 * 0 .. 3n + 1 and a non-finite local point -- each with its index.
 * ------------------------------------------------------------------------------------------------------------------- */
#define SNK_BIAS_VELOCITY 1     /* flags: the velocity-product (Coriolis, centrifugal, gyroscopic) terms of h */
#define SNK_BIAS_GRAVITY  2     /* flags: minus the generalised gravity force */
#define SNK_JAC_MAX_POINTS 256  /* points of one snk_jacobians call */
int32_t snk_dyn_dofs(const snk_handle* h);
int snk_dynamics(snk_handle* h, const int32_t* env_ids_dev, int32_t n_rows, int32_t flags, float* mass_dev, float* bias_dev,
                 void* stream);
int snk_dynamics_host(snk_handle* h, const int32_t* env_ids, int32_t n_rows, int32_t flags, float* mass, float* bias);
int snk_jacobians(snk_handle* h, const int32_t* env_ids_dev, int32_t n_rows, const int32_t* link_rows_dev, const float* local_dev,
                  int32_t n_points, float* jac_dev, void* stream);
int snk_jacobians_host(snk_handle* h, const int32_t* env_ids, int32_t n_rows, const int32_t* link_rows, const float* local,
                       int32_t n_points, float* jac);

/* ---------------------------------------------------------------------------------------------------------------------
 * The applied forces: the contract of snk_apply_impulse (what PyBullet exposes as applyExternalForce, applyExternalTorque
 * and TORQUE_CONTROL, which the reference never calls and a controller computing tau = h + J^T f from the dynamics
 * queries, or a trainer pushing a link for a few substeps, does).  The kernel (bullet-envs_amd/csrc/snk_dyn.hpp:
 * impulse_kernel) and the independent numpy model of the tests (tests/np_impulse.py) are both written from this text.
 *
 * What it is.  Forward dynamics is affine in the applied force: ABA(q, u, Q) = ABA(q, u, 0) + M(q)^-1 Q.  A generalised
 * force Q held for `seconds` is therefore, to first order, the velocity impulse delta = seconds x M(q)^-1 Q, and this call
 * adds it to the velocity the state holds NOW, by a kernel of its own, in front of whatever steps next (snk_substep,
 * snk_step, the fused env-step): the step kernels do not know of it.  With max_motor_impulse = 0 in snk_params (motors
 * off) it is TORQUE_CONTROL; with the default motors it is a push on a servo-held snake.
 *
 * Q = gen_force + sum_p J_p^T [f_p ; tau_p], in the coordinates of "The dynamics queries":
 *   gen_force_dev [n_envs][nd] f32 or NULL: the generalised force conjugate to u = [omega | v | qd] -- the moment about the
 *     root link's origin (world axes) 3, the force 3, the joint torques n; Q . u is power.
 *   link_rows_dev [n_points] i32: rows of snk_link_states, ONE list shared by every env (as in snk_jacobians); n_points in
 *     0 .. SNK_IMPULSE_MAX_POINTS, with 0 both pointers may be NULL.  A row may repeat: its wrenches add up.
 *   wrench_dev [n_envs][n_points][SNK_WRENCH_FLOATS] f32: [force 3 | torque 3 | point 3] per env and point.  Without
 *     SNK_IMPULSE_LINK_FRAME (PyBullet's WORLD_FRAME) force and torque are in world axes and the point is a world position
 *     that rides on the link for this call; with it (LINK_FRAME) all three are in the link's COM frame, the frame of
 *     snk_jacobians' local_dev: origin the link's COM, axes the link's rotation.  J_p is exactly the Jacobian
 *     snk_jacobians reports for that link and point.  A link row outside 0 .. 3n + 1 cannot be refused on the device
 *     path: it contributes nothing.
 *   A call with neither gen_force_dev nor points is refused.
 * delta = seconds x M(q)^-1 Q, M the matrix snk_dynamics reports: rigid bodies only, no damping and no h -- a caller who
 * wants unconstrained forward dynamics passes Q - h.  It is computed by the articulated-body recursion of the substep
 * itself, never by factoring the dense M.  seconds must be finite and >= 0.  delta_dev [n_envs][nd] f32 or NULL.
 *
 * What is written.  active_dev [n_envs] u8 or NULL (all envs): snk_substep's mask, not an id list -- the call writes state
 * and repeated ids would race.  An env whose byte is 0 is neither loaded nor stored and its row of delta is zeros.  Of an
 * active env the velocity floats of the record -- floats 7-12 and 13 + n .. 12 + 2n of snk_get_state -- become u + delta,
 * ONE float32 add per component, and nothing else is written: pose, q, the aux floats (motor torques, joint-0 force,
 * previous x), the contact cache, the free box, the ground friction and the reset poses keep their bits.  With
 * SNK_IMPULSE_DRY the arithmetic is the same and nothing of the state is written: delta_dev (required then) is the
 * impulse response M^-1 Q x seconds.  No clamp is applied: the next substep's max_coord_vel rule sees the new velocity.
 * The free box of obstacle 2 cannot be pushed: it is a body of its own with no component in u, and is out of scope here.
 *
 * [U] Next to Bullet.  Bullet puts an applied force into the SAME articulated-body pass as -h(q, u) and the damping; here
 * the step that follows evaluates those at u + delta instead of u.  The difference is dt x d(h + damping)/du x delta:
 * second order in dt (measured: DESIGN.md 3, "Other deviations"; tests/test_np_impulse.py prints it).
 *
 * Asynchronous on `stream`, one launch (one wave per env), no atomics, no waits, nothing allocated: it can be captured in
 * a graph.  It does not synchronise, copy or validate.  Refused, naming the argument: a null or poisoned handle; unknown
 * flag bits; n_points out of range; points without link_rows_dev or without wrench_dev; nothing to apply;
 * SNK_IMPULSE_DRY without delta_dev; seconds negative or not finite; a pointer that is not 4-byte aligned.
 * snk_apply_impulse_host: the same with HOST buffers; it synchronises the device first, like the state accessors, and also
 * refuses a link row outside 0 .. 3n + 1 and, in the rows of the active envs, a non-finite generalised force, wrench or
 * point -- each with its index.
 * ------------------------------------------------------------------------------------------------------------------- */
#define SNK_WRENCH_FLOATS 9          /* [force 3 | torque 3 | point 3] */
#define SNK_IMPULSE_LINK_FRAME 1     /* flags: force, torque and point are in the link's COM frame (PyBullet's LINK_FRAME);
                                        without it world axes and a world point (WORLD_FRAME) */
#define SNK_IMPULSE_DRY 2            /* flags: compute delta only, write nothing of the state */
#define SNK_IMPULSE_MAX_POINTS 256   /* points of one snk_apply_impulse call */
int snk_apply_impulse(snk_handle* h, const uint8_t* active_dev, const float* gen_force_dev, const int32_t* link_rows_dev,
                      const float* wrench_dev, int32_t n_points, int32_t flags, float seconds, float* delta_dev, void* stream);
int snk_apply_impulse_host(snk_handle* h, const uint8_t* active, const float* gen_force, const int32_t* link_rows,
                           const float* wrench, int32_t n_points, int32_t flags, float seconds, float* delta);

/* Where this build's structural limits were met, counted on the device since snk_create (Bullet has no such limits;
 * DESIGN.md 3).  Ground contacts have none left: the streamed-row solve has a slot for every point its chain's manifolds
 * can hold (8n), and the register-resident 16-link solve hands the substeps that outgrow its 64 slots to it.
 *   out[0] 16-link handles on the register-resident solve: physics substeps in which an environment held more contact
 *          points than that solve's 64 slots (a snake at rest gathers up to four per cylinder), touched the
 *          obstacle with more than eight cylinders, or had two of its links within reach of each other (that
 *          solve has no two-body rows).  Those substeps are
 *          solved by the streamed-row solve of the same chain instead, in the same launch, with every point -- a
 *          count of slower substeps, not of lost contacts.  Streamed-row handles: always 0,
 *   out[1] manifold points that got no rows: always 0 (kept as a tripwire: the finders still count against the slots),
 *   out[2] link-link / obstacle contacts beyond the room for them (32 in all; obstacle contacts are kept before
 *          link-link ones): a 32-link chain can reach it; a 16-link one only when tangled beyond its joint limits with
 *          more than 32 pairs of links touching at once (states set from outside: tests/test_gpu_accuracy_distribution.py
 *          meets 6 in 1024 random foldings) -- a substep with more than the register-resident solve's eight box contacts
 *          goes through the other solve, which has room for every cylinder.
 * Host buffer of 3. */
int snk_contact_overflow(snk_handle* h, uint64_t* out);

/* How many contact points the environments held, physics substep by physics substep, since snk_create (or the last
 * reset of these counters): out[k] = substeps that ran with k contact points (ground + link-link + obstacle), the last
 * bin collecting everything beyond it.  snk_contact_histogram_bins() values (host buffer).  This is the distribution
 * that sizes the register-resident solve's row slots; counted by the step and the substep kernels alike
 * -- while enabled (snk_contact_histogram_enable).  reset != 0 zeroes the counters after reading. */
int32_t snk_contact_histogram_bins(void);
int snk_contact_histogram(snk_handle* h, uint64_t* out, int32_t reset);
/* The counting is OFF after snk_create (it costs one atomic per physics substep: 0.7 % of the headline rate) and is
 * switched with this call; the counters keep what they hold. */
int snk_contact_histogram_enable(snk_handle* h, int32_t on);

/* BASELINE config 5: per-env lateral friction of the ground plane (reference: plane.urdf = 1). */
int snk_set_ground_friction(snk_handle* h, const float* mu /* host [n_envs] */);
int snk_get_ground_friction(snk_handle* h, float* mu /* host [n_envs] */);

/* Test hook: sets the step queue's ticket counters (in-launch scheduling) to `base`, so that a test
 * can put the wrap-around of the 32-bit tickets inside its next step.  Results never depend on it. */
int snk_debug_set_tickets(snk_handle* h, uint32_t base);

/* Test hook for the failure path: raises this handle's alarm from the HOST -- the host-mapped word a wave of the step
 * kernel sets when one of its bounded waits runs out (nothing waits, nothing hangs).  Afterwards the handle behaves as
 * after a real alarm: snk_step / snk_step_packed / snk_step_traced(_host) / snk_step_host / snk_reset(_host) / snk_substep_host and the state
 * accessors (get/set state, manifold, box, obs, mean height, link positions, joint-3 force, set_ground_friction,
 * snk_set_reset_pose, snk_get_reset_pose, snk_set_reset_pose_dev) and snk_render / snk_render_host and the tensor seam
 * (snk_substep, snk_observe, snk_link_states(_host), snk_copy_envs(_host), snk_contacts(_host), snk_closest_points(_host)) and snk_ray_test(_host) and snk_dynamics(_host) and snk_jacobians(_host) and snk_apply_impulse(_host) return
 * non-zero -- and snk_reset_pose_floats, snk_contact_slots, snk_link_pairs, snk_closest_slots and snk_dyn_dofs 0 -- with snk_last_error() = "env-step scheduler: a bounded wait ran out ..."; snk_destroy succeeds.  The
 * reference's failure story is SubprocVecEnv.close() draining and joining its workers
 * (ppo/multiprocessing_env.py:140-150): here too the only way on is to destroy the handle and create a new one. */
int snk_debug_raise_alarm(snk_handle* h);

/* Test hook (host only, no handle): the 2 n-entry sweep order the kernels are compiled with for noncontact_order 1 and
 * n_modules n (16 or 32), in the oracle's convention (orc_quicksort_equal_keys over 2 n): out[k] = the row at place k of
 * the forward sweep, entries 0..n-1 naming limit j, entries n..2n-1 motor j - n.  Read from the same constexpr table
 * the kernels unroll their sweeps over. */
int snk_debug_noncontact_order(int32_t n_modules, int32_t* out);

/* Test hooks: the streamed-row solve's intermediate results ("stage by stage").  That solve keeps its
 * constraint rows in a block of global memory per resident workgroup (snk_lds.hpp: Lds<N, false>): every normal and
 * friction record, the 20-float geometry of every contact slot, M^-1 and the Y block behind it.
 * snk_debug_rows_layout (host only, no handle): the 14 constants of that layout for n_modules 16 or 32, out[14] =
 * [ND, NC, NCT, kRows, kFric, kRS, kMO, kSpec, kGeo, kGeoOff, kMmOff, kYOff, kRowFloats, kBoxBody].
 * snk_debug_rows: waits for the device and copies block `env`, kRowFloats floats, as the last substep of that environment
 * left it.  It refuses, with a message that says which, unless the handle runs the streamed-row kernels (32 links,
 * obstacle 2, SNK_FORCE_STREAMED), holds no more environments than resident waves, and the last launch on it was
 * snk_substep_host, or snk_substep with a null mask: only then has workgroup b run environment b and nothing else (a
 * masked snk_substep skips environments, whose blocks keep what an earlier launch left: it counts as another launch).
 * Device code is not involved. */
int snk_debug_rows_layout(int32_t n_modules, int32_t* out);
int snk_debug_rows(snk_handle* h, int32_t env, float* out /* host, kRowFloats */);

/* Test hook (host only, no handle): what the kernels' bound on one substep's change of the mean height is made of for
 * this parameter set ("when the sensor pass runs"): out[0] = the longest joint-to-joint offset of the chain
 * and out[1] = the distance of the base link's COM from the root origin, both in metres and rounded up by 1.001 as the
 * device model holds them; out[2] = the bound's fixed slack in metres. */
int snk_debug_reach_bound(const snk_params* p, float out[3]);

/* Device-side self test of the wave primitives (DPP reductions); 0 = pass. */
int snk_selftest(int32_t device);

/* Dominant-kernel timing with HIP events on the launch stream: enable(capacity) arms a pool
 * of `capacity` event pairs (0 disarms); each following snk_step launch is bracketed by one
 * pair, without any host synchronisation; read() waits for them, returns the mean launch
 * duration in ms and how many launches it covers, and re-arms the pool. */
int snk_timing_enable(snk_handle* h, int32_t capacity);
int snk_timing_read(snk_handle* h, double* mean_ms, int32_t* count);

/* What the kernels derive from a parameter set, without a device (host arithmetic only), for tests: out[6] =
 * [contact breaking threshold of a (ground | link | box, link) manifold in metres (relative_breaking_threshold 1:
 *  breaking_threshold x the link collider's angular-motion disc), collision cylinder radius, half length, centre along
 *  the link's z (snake.urdf:806-811), collision margin, breaking threshold of the (ground, box) manifold]. */
int snk_params_derived(const snk_params* p, double* out);

/* Merged-model introspection for tests: per composite body [mass, com3, I_origin6] and
 * rest-pose world origins.  out_bodies [(n+1) x 10], out_origins [(n+1) x 3] (host). */
int snk_model_describe(const snk_handle* h, double* out_bodies, double* out_origins);

const char* snk_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
