"""The INNER seam of the reference: `Snake(pybullet_client, urdf_root, args)` takes its physics engine as an
injected object (/root/reference/snake.py:14-18) and calls ~20 PyBullet functions on it (snake.py:79-330).  This module
is that object, answered by the HIP kernels behind include/snk.h -- one client = one world = one environment, like the
one PyBullet connection each of the reference's env processes owns (SnakeGymEnv.py:23 -> snake.py:89):

    from bullet_envs_amd import BulletClient            # instead of `import pybullet as p`
    p = BulletClient()                                   # p.connect(p.DIRECT) is accepted and does nothing
    robot = Snake(p, "snake/snake.urdf", args)           # the REFERENCE's own snake.py, unmodified
    env = SnakeGymEnv(robot, args)                       # the reference's own SnakeGymEnv.py

Every stepSimulation() is one launch of the single-substep kernel (snk_substep_host) and every read-out a device
synchronisation, so this is a COMPATIBILITY shim -- the reference's Python loop stays the bottleneck (49 getJointState
calls per observation, snake.py:180-206).  The performant seams are the VecEnv (snake_env.py: SnakeVecEnv) and the
device-resident DeviceVecEnv; what this one buys is that the reference's env logic can run on this engine line for
line, which is also how tests check that the fused env-step kernel IS that logic (tests/test_pybullet_client.py).

Only what the path calls is implemented; anything else raises AttributeError (no silent stubs).  The world is created
lazily, at the first call that needs it, from what loadURDF / changeDynamics / setGravity / setTimeStep said before.

getLinkStates stays what the path reads: the COM positions of links 0, 3, ..., 3n, a placeholder in the orientation's
place, any other link refused (tests/test_pybullet_client.py pins both, and its CPU stand-in answers link_positions
only).  The orientations, origins and velocities of ALL 3n + 2 links are one level down: Stepper.link_states /
DeviceWorld.link_states (snk_link_states), and Snake.getLinkOrientations / getBaseVelocity of snake_env.py.

getContactPoints answers what the handle holds: the ground contacts of the snake and of the free block, from the contact
cache (snk_contacts).  Link-link and link-block contacts are stateless in the kernels: a query for them is refused.

getClosestPoints answers (snake, block) and (snake, snake) at a caller-given distance: the solver's narrow phase run as a
query on the current pose (snk_closest_points), one point per pair, no forces.  Distances to the plane are refused.

rayTest / rayTestBatch cast rays against the plane, the snake's link colliders and the block at the current pose
(snk_ray_test): world rays, or rays riding on a link of the snake (parentObjectUniqueId, parentLinkIndex).
"""
import math
import os

import numpy as np

from . import _lib


class BulletClient(object):
    # the constants the path reads off the client
    POSITION_CONTROL = 2
    URDF_USE_SELF_COLLISION = 8
    DIRECT = 2
    GUI = 1
    ER_SEGMENTATION_MASK_OBJECT_AND_LINKINDEX = 1
    ER_TINY_RENDERER = 65536
    ER_BULLET_HARDWARE_OPENGL = 131072

    _PLANE, _SNAKE, _BLOCK = 0, 1, 2

    def __init__(self, device=0, n_modules=16, render=None, **params):
        if render not in (None, 'kernel'):
            raise ValueError("render must be None or 'kernel', got %r" % (render,))
        self._render = render                # 'kernel': getCameraImage draws (snk_render); None: PyBullet's 5-tuple, no pixels
        self._camera = {}                    # what the last resetDebugVisualizerCamera said
        self._device = device
        self._n = n_modules
        self._over = dict(params)
        self._st = None
        self._forget_world()

    # ---- connection / world building (ppo/train.py:60; snake.py:88-107; snake_gait_test.py:44-53) ----
    def connect(self, mode=None, *a, **k):
        return 0

    def disconnect(self, *a, **k):
        self.close()

    def close(self):
        if self._st is not None:
            self._st.close()
            self._st = None

    def _forget_world(self):
        self.close()
        self._world = dict(self._over)       # snk_params overrides collected until the world is built
        self._bodies = {}
        self._targets = None
        self._cache = None

    def resetSimulation(self):
        self._forget_world()

    def setAdditionalSearchPath(self, path):
        return None

    def setGravity(self, x, y, z):
        if x != 0 or y != 0:
            raise NotImplementedError("BulletClient: gravity along z only (snake.py:91)")
        self._set("gravity_z", float(z))

    def setTimeStep(self, dt):                           # snake.py:271-272 (never called on the training path), snake_gait_test.py:53
        self._set("dt", float(dt))

    def _set(self, key, value):
        if self._st is not None and self._world.get(key) != value:
            raise RuntimeError("BulletClient: %s changed after the world was built; call resetSimulation() first" % key)
        self._world[key] = value

    def loadURDF(self, fileName, basePosition=None, baseOrientation=None, useFixedBase=0, flags=0, **kw):
        name = os.path.basename(str(fileName))
        if name == "plane.urdf":
            self._bodies[self._PLANE] = "plane"
            return self._PLANE
        if name.startswith("block"):                     # snake/block.urdf (snake.py:83-84, snake_gait_test.py:51)
            self._set("obstacle", 1 if useFixedBase else 2)
            self._set("obstacle_pos", [float(v) for v in (basePosition or (2.0, 0.0, 0.1))])
            self._bodies[self._BLOCK] = "block"
            return self._BLOCK
        if "snake" in name:
            if basePosition is not None and any(float(v) != 0.0 for v in basePosition):
                raise NotImplementedError("BulletClient: the snake is loaded at the origin (snake.py:93)")
            if useFixedBase:
                raise NotImplementedError("BulletClient: floating base only (snake.py:93)")
            self._set("self_collision", 1 if (flags & self.URDF_USE_SELF_COLLISION) else 0)
            self._bodies[self._SNAKE] = "snake"
            return self._SNAKE
        raise NotImplementedError("BulletClient: no model for %r (plane.urdf, snake.urdf, block.urdf)" % fileName)

    def changeDynamics(self, body, link, lateralFriction=None, anisotropicFriction=None, **kw):
        if kw:
            raise NotImplementedError("BulletClient.changeDynamics: %s" % sorted(kw))
        if body == self._SNAKE:                          # snake.py:103-106: the same values for the base and every link
            if lateralFriction is not None:
                self._set("mu_link", float(lateralFriction))
            if anisotropicFriction is not None:
                self._set("aniso", [float(v) for v in anisotropicFriction])
        elif body == self._BLOCK and lateralFriction is not None:
            self._set("mu_obstacle", float(lateralFriction))

    # what snake_gait_test.py:20-26,54-55,73-74 calls besides: accepted, nothing to do on this engine (no GUI, no real-time
    # clock); getCameraImage hands back PyBullet's 5-tuple with no pixels
    def setRealTimeSimulation(self, enable):
        if enable:
            raise NotImplementedError("BulletClient: stepSimulation drives the clock (snake_gait_test.py:54)")

    def resetDebugVisualizerCamera(self, cameraDistance=None, cameraYaw=None, cameraPitch=None, cameraTargetPosition=None,
                                   *a, **k):
        if self._render is not None:         # remembered: the camera of a getCameraImage without matrices [U]
            self._camera = dict(distance=cameraDistance, yaw=cameraYaw, pitch=cameraPitch, target=cameraTargetPosition)
        return None

    def computeViewMatrixFromYawPitchRoll(self, cameraTargetPosition, distance, yaw, pitch, roll, upAxisIndex, *a, **k):
        """snake.py:310-316.  PyBullet's 16-tuple (column-major), from snk_view_matrix_ypr [U]."""
        if self._render is None:
            raise AttributeError("BulletClient(render=None) has no computeViewMatrixFromYawPitchRoll: pass render='kernel'")
        return tuple(float(v) for v in _lib.view_matrix_ypr(cameraTargetPosition, distance, yaw, pitch, roll, upAxisIndex))

    def computeProjectionMatrixFOV(self, fov, aspect, nearVal, farVal, *a, **k):
        """snake.py:317-320 (which passes farVal = nearVal: the entries come out infinite, nothing raises).  PyBullet's
        16-tuple, from snk_projection_fov [U]."""
        if self._render is None:
            raise AttributeError("BulletClient(render=None) has no computeProjectionMatrixFOV: pass render='kernel'")
        return tuple(float(v) for v in _lib.projection_fov(fov, aspect, nearVal, farVal))

    def default_camera(self, width, height):
        """(view, proj) of a getCameraImage without matrices [U]: the last resetDebugVisualizerCamera (before any: the
        reference's own, snake.py:322-325) with fov 60, near 0.01, far 100 -- _lib.DEFAULT_CAMERA says why."""
        c = {k: v for k, v in self._camera.items() if v is not None}
        return _lib.default_camera(width, height, **c)

    def segmentation_ids(self, seg, flags=0):
        """Primitive ids of snk_render (0 ground, 1 + c cylinder c, 1 + 2n box, -1 none) -> PyBullet's: the body ids this
        client hands out (plane 0, snake 1, block 2), and under ER_SEGMENTATION_MASK_OBJECT_AND_LINKINDEX
        + ((link index + 1) << 24) with the cylinder's Bullet link (INPUT_INTERFACE_k = 3k - 2, OUTPUT_BODY_k = 3k; the
        plane and the block are base links, -1)."""
        seg = np.asarray(seg)
        n = self._n
        c = seg - 1
        out = np.where(seg == 0, self._PLANE, np.where(seg == 1 + 2 * n, self._BLOCK, self._SNAKE)).astype(np.int32)
        if flags & self.ER_SEGMENTATION_MASK_OBJECT_AND_LINKINDEX:
            link = np.where(c % 2 == 0, 3 * (c // 2 + 1) - 2, 3 * ((c + 1) // 2))
            out = out + np.where((seg >= 1) & (seg <= 2 * n), (link + 1) << 24, 0).astype(np.int32)
        return np.where(seg < 0, -1, out).astype(np.int32)

    def getCameraImage(self, width, height, viewMatrix=None, projectionMatrix=None, shadow=0, flags=0, *a, **k):
        """snake.py:326-327, snake_gait_test.py:19-26.  render=None: PyBullet's 5-tuple with no pixels, as before.
        render='kernel': (width, height, rgba (h, w, 4) uint8, depth (h, w) float32, segmentation (h, w) int32)."""
        if self._render is None:
            return (width, height, [], [], [])
        if viewMatrix is None or projectionMatrix is None:
            dv, dp = self.default_camera(width, height)
            viewMatrix = dv if viewMatrix is None else viewMatrix
            projectionMatrix = dp if projectionMatrix is None else projectionMatrix
        rgba, dep, seg = self._stepper().render(viewMatrix, projectionMatrix, width, height, shadow=bool(shadow))
        return (width, height, rgba[0], dep[0], self.segmentation_ids(seg[0], flags))

    def getJointInfo(self, body, joint):
        """(index, name, type, ...) in PyBullet's layout, from the URDF's module pattern: joint 3k is
        module k's revolute joint (type 0), the others are fixed (type 4)."""
        if body != self._SNAKE or not (0 <= joint <= 3 * self._n):
            raise NotImplementedError("BulletClient.getJointInfo: the snake's joints 0 .. 3n")
        if joint == 0:
            name, link, k = "base_joint", "base", 0
        else:
            k = (joint + 2) // 3
            part = ("INPUT_INTERFACE", "COLLAR", "OUTPUT_BODY")[(joint - 1) % 3]
            name, link = "SA%03d_%s_joint" % (k, part), "SA%03d_%s" % (k, part)
        rev = joint >= 3 and joint % 3 == 0
        lo, hi = (self._world.get("joint_lo", -1.57), self._world.get("joint_hi", 1.57)) if rev else (0.0, -1.0)
        return (joint, name.encode(), 0 if rev else 4, (6 + k if rev else -1), (5 + k if rev else -1), 1,
                0.1 if rev else 0.0, 0.2 if rev else 0.0, lo, hi, 7.0 if rev else 0.0, 2.208932 if rev else 0.0,
                link.encode(), (0.0, 1.0, 0.0) if rev else (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0), joint - 1)

    def enableJointForceTorqueSensor(self, body, joint, enableSensor=1):
        return None                                      # joints 0 and 3 are always evaluated (obs[55]; snake_gait_test.py:126)

    def getNumJoints(self, body):
        return 3 * self._n + 1 if body == self._SNAKE else 0

    # ---- the world itself ----
    def _stepper(self):
        if self._st is None:
            if self._SNAKE not in self._bodies:
                raise RuntimeError("BulletClient: no snake loaded (loadURDF) yet")
            self._st = _lib.Stepper(1, device=self._device, n_modules=self._n, **self._world)
            self._targets = np.zeros((1, self._n), dtype=np.float32)
            self._cache = None
        return self._st

    def _state(self):
        """(state, aux, link positions) of the world, fetched once per simulator state."""
        if self._cache is None:
            st = self._stepper()
            s, x = st.get_state()
            self._cache = (s[0].astype(np.float64), x[0].astype(np.float64), None)
        return self._cache

    def _motor(self, joint):
        if joint % 3 != 0 or not (3 <= joint <= 3 * self._n):
            raise NotImplementedError("BulletClient: joint %d is not a motor joint (3, 6, ..., 3n)" % joint)
        return joint // 3 - 1

    # ---- reset (snake.py:119-127) ----
    def resetBasePositionAndOrientation(self, body, posObj, ornObj):
        st = self._stepper()
        s, _ = st.get_state()
        s[0, 0:3] = posObj
        s[0, 3:7] = ornObj
        s[0, 7:13] = 0.0                                 # [U] zeroes the base twist
        st.set_state(s)
        self._cache = None

    def resetJointState(self, body, jointIndex, targetValue, targetVelocity=0.0):
        j = self._motor(jointIndex)
        st = self._stepper()
        s, _ = st.get_state()
        s[0, 13 + j] = targetValue
        s[0, 13 + self._n + j] = targetVelocity
        st.set_state(s)
        self._cache = None

    # ---- the substep (snake.py:219-221, 286) ----
    def _check_forces(self, forces):
        if forces is None:
            return
        f = np.asarray(forces, dtype=np.float64).reshape(-1)
        mi = self._world.get("max_motor_impulse", math.inf)
        dt = self._world.get("dt", 1.0 / 240.0)
        want = math.inf if np.all(np.isinf(f)) else float(f[0]) * dt
        if not np.all(f == f[0]):
            raise NotImplementedError("BulletClient: one force limit for all motors (snake.py:26-27)")
        if want != mi:
            self._set("max_motor_impulse", want)         # fine before the world exists, an error after

    def setJointMotorControlArray(self, bodyUniqueId, jointIndices, controlMode, targetPositions=None, forces=None, **kw):
        if controlMode != self.POSITION_CONTROL or kw:
            raise NotImplementedError("BulletClient: POSITION_CONTROL with PyBullet's default gains only (snake.py:221)")
        self._check_forces(forces)
        self._stepper()
        for j, t in zip(jointIndices, targetPositions):
            self._targets[0, self._motor(j)] = t

    def setJointMotorControl2(self, bodyIndex, jointIndex, controlMode, targetPosition=0.0, force=None, **kw):
        # snake_gait_test.py:71-76 drives the motors one by one (its positionGain / velocityGain are PyBullet's defaults
        # spelt out); snake.py:109-117's kp = 10 form is not on the path and not supported
        if controlMode != self.POSITION_CONTROL:
            raise NotImplementedError("BulletClient: POSITION_CONTROL only")
        if kw.get("positionGain", 0.1) != 0.1 or kw.get("velocityGain", 1.0) != 1.0:
            raise NotImplementedError("BulletClient: PyBullet's default gains only (kp 0.1, kd 1.0)")
        self._check_forces(None if force is None else [force])
        self._stepper()
        self._targets[0, self._motor(jointIndex)] = targetPosition

    def stepSimulation(self):
        self._stepper().substep(self._targets, 1)
        self._cache = None

    # ---- read-out (snake.py:130-146, 180-206, 237-245; snake_gait_test.py:33-40) ----
    def getJointState(self, bodyUniqueId, jointIndex):
        s, x, _ = self._state()
        n = self._n
        if jointIndex == 0:                              # the head sensor: obs[55] = reaction Fz (snake.py:202-206)
            return (0.0, 0.0, (0.0, 0.0, float(x[n]), 0.0, 0.0, 0.0), 0.0)
        j = self._motor(jointIndex)
        # the 6-D reaction is evaluated for joints 0 and 3 only (obs[55]; snake_gait_test.py:126 reads joint 3's Fz and
        # records the others without using them): the rest come back as NaN, not as a made-up zero
        nan = float("nan")
        react = (nan,) * 6
        if jointIndex == 3:
            react = (nan, nan, float(self._stepper().joint3_reaction_fz()[0]), nan, nan, nan)
        return (float(s[13 + j]), float(s[13 + n + j]), react, float(x[j]))

    def getBasePositionAndOrientation(self, bodyUniqueId):
        s, _, _ = self._state()
        return tuple(float(v) for v in s[0:3]), tuple(float(v) for v in s[3:7])

    def getLinkStates(self, bodyUniqueId, linkIndices, **kw):
        idx = [int(i) for i in linkIndices]
        if any(i % 3 != 0 or not (0 <= i <= 3 * self._n) for i in idx):
            raise NotImplementedError("BulletClient.getLinkStates: links 0, 3, ..., 3n (snake.py:142, 240)")
        s, x, lp = self._state()
        if lp is None:
            lp = self._stepper().link_positions()[0].astype(np.float64).reshape(3, self._n + 1)      # [x.., y.., z..]
            self._cache = (s, x, lp)
        # [0] = world position of the link's COM: the only field the path reads.  (PyBullet's further fields are 3- and
        # 4-vectors; snake.py:143 builds an array from the tuples, which numpy >= 1.24 only accepts when they have one
        # length -- hence a 3-vector placeholder in the orientation's place)
        return [((float(lp[0, i // 3]), float(lp[1, i // 3]), float(lp[2, i // 3])), (0.0, 0.0, 0.0)) for i in idx]

    def getContactPoints(self, bodyA=-1, bodyB=-1, linkIndexA=-2, linkIndexB=-2, **kw):
        """PyBullet's list of 14-tuples (contactFlag, bodyA, bodyB, linkIndexA, linkIndexB, positionOnA, positionOnB,
        contactNormalOnB, distance, normalForce, lateralFriction1, lateralFrictionDir1, lateralFriction2,
        lateralFrictionDir2) for the pair (snake, plane) or (block, plane), given in either order and never swapped -- A is
        the snake (or the block), B the plane, the ids those loadURDF returned: the live slots of snk_contacts, in slot
        order (include/snk.h, "The reported contacts").  The positions are those of the CURRENT pose (PyBullet: of the
        last collision pass), the normal force that of the last substep.  [U] The four lateral-friction entries are zeros: the kernels store no friction impulse per point.
        linkIndexA / linkIndexB (-2: any) filter by the link on their side; the plane's and the block's link is -1.
        Refused (NotImplementedError): a query that leaves the pair open, and snake-snake or snake-block pairs -- those
        contacts are stateless in the kernels, the handle does not hold them."""
        if kw:
            raise NotImplementedError("BulletClient.getContactPoints: %s" % sorted(kw))
        pair = (bodyA, bodyB)
        if self._PLANE not in pair or bodyA == bodyB or not all(b in self._bodies for b in pair):
            raise NotImplementedError(
                "BulletClient.getContactPoints: only (snake, plane) and (block, plane) are held by the handle (the contact "
                "cache); got bodyA=%r, bodyB=%r -- link-link and link-block contacts are stateless in the kernels and not "
                "stored, and a query that leaves a body open would have to list them" % (bodyA, bodyB))
        mover = bodyA if bodyB == self._PLANE else bodyB
        st = self._stepper()
        points = st.contacts()[0][0].astype(np.float64)
        n = self._n
        if mover == self._SNAKE:
            rows = points[:8 * n]
            links = np.repeat(np.asarray(st.contact_links(), dtype=np.int64), 4)
        else:
            rows = points[8 * n:]
            links = np.full(len(rows), -1, dtype=np.int64)
        # the filters belong to the bodies as the query names them; the tuples are never swapped: A is the moving body
        want_mover, want_plane = (linkIndexB, linkIndexA) if bodyA == self._PLANE else (linkIndexA, linkIndexB)
        if want_plane not in (-2, -1):
            return []
        zero3 = (0.0, 0.0, 0.0)
        return [(0, mover, self._PLANE, int(link), -1, tuple(float(v) for v in r[0:3]), tuple(float(v) for v in r[3:6]),
                 tuple(float(v) for v in r[6:9]), float(r[9]), float(r[10]), 0.0, zero3, 0.0, zero3)
                for r, link in zip(rows, links) if r[14] != 0.0 and want_mover in (-2, link)]

    def getClosestPoints(self, bodyA, bodyB, distance, linkIndexA=-2, linkIndexB=-2, **kw):
        """PyBullet's list of 14-tuples (getContactPoints' layout) for the pair (snake, block) or (snake, snake): the pairs
        closer than `distance` at the CURRENT pose, one point per pair (PyBullet: up to four, as of the last collision pass)
        -- the live slots of snk_closest_points in slot order (include/snk.h, "The closest points").  normalForce and the
        four lateral-friction entries are zeros: these contacts carry no stored impulse.  The pair may be given in either
        order and the tuples are never swapped: A is the snake's cylinder a, B the block (link -1) or cylinder b > a; the
        links are those of contact_links().  linkIndexA / linkIndexB (-2: any) filter by the link of the body they are
        given for; in a (snake, snake) query linkIndexA filters A's link and linkIndexB B's.
        Refused (NotImplementedError): pairs with the plane, unknown bodies, extra keywords."""
        if kw:
            raise NotImplementedError("BulletClient.getClosestPoints: %s" % sorted(kw))
        pair = (bodyA, bodyB)
        if (self._PLANE in pair or self._SNAKE not in pair or not all(b in self._bodies for b in pair)
                or pair == (self._BLOCK, self._BLOCK)):
            raise NotImplementedError(
                "BulletClient.getClosestPoints: only (snake, block) and (snake, snake) are answered (snk_closest_points); got "
                "bodyA=%r, bodyB=%r -- distances to the plane are not computed" % (bodyA, bodyB))
        st = self._stepper()
        n = self._n
        links = np.asarray(st.contact_links(), dtype=np.int64)
        zero3 = (0.0, 0.0, 0.0)
        if bodyA == bodyB:
            rows = st.closest_points(distance, flags=_lib.PAIRS_LINKS)[0][0][2 * n:].astype(np.float64)
            other, want_a, want_b = self._SNAKE, linkIndexA, linkIndexB
            link_b = lambda r: int(links[int(r[13])])      # noqa: E731
        else:
            rows = st.closest_points(distance, flags=_lib.PAIRS_BOX, max_pairs=0)[0][0].astype(np.float64)
            other = self._BLOCK
            want_a, want_b = (linkIndexA, linkIndexB) if bodyA == self._SNAKE else (linkIndexB, linkIndexA)
            link_b = lambda r: -1                          # noqa: E731
        return [(0, self._SNAKE, other, int(links[int(r[12])]), link_b(r), tuple(float(v) for v in r[0:3]),
                 tuple(float(v) for v in r[3:6]), tuple(float(v) for v in r[6:9]), float(r[9]), 0.0, 0.0, zero3, 0.0, zero3)
                for r in rows if r[14] != 0.0 and want_a in (-2, int(links[int(r[12])])) and want_b in (-2, link_b(r))]

    def rayTestBatch(self, rayFromPositions, rayToPositions, parentObjectUniqueId=-1, parentLinkIndex=-1, **kw):
        """PyBullet's list of (objectUniqueId, linkIndex, hitFraction, hitPosition, hitNormal), one per ray, from
        snk_ray_test on the CURRENT pose (include/snk.h, "The ray test"): the first solid each ray enters -- the plane (body
        0, link -1), a link collider of the snake (body 1, the cylinder's link of contact_links()) or the block (body 2,
        link -1); a miss is (-1, -1, 1.0, zeros, zeros).  With parentObjectUniqueId = the snake the rays are in the frame
        of link parentLinkIndex (-1: the base), its origin the link's COM [U], and ride on it; positions and normals come
        back in world coordinates either way.
        Refused (NotImplementedError): a parent other than the snake, extra keywords (numThreads, reportHitNumber,
        collisionFilterMask, fractionEpsilon)."""
        if kw:
            raise NotImplementedError("BulletClient.rayTestBatch: %s" % sorted(kw))
        if parentObjectUniqueId not in (-1, self._SNAKE) or (parentObjectUniqueId == -1 and parentLinkIndex != -1):
            raise NotImplementedError("BulletClient.rayTestBatch: rays ride on the snake's links only; got "
                                      "parentObjectUniqueId=%r, parentLinkIndex=%r" % (parentObjectUniqueId, parentLinkIndex))
        frm = np.asarray(rayFromPositions, dtype=np.float32).reshape(-1, 3)
        to = np.asarray(rayToPositions, dtype=np.float32).reshape(-1, 3)
        if len(frm) != len(to):
            raise ValueError("rayFromPositions and rayToPositions must name as many points each, got %d and %d" % (len(frm), len(to)))
        if len(frm) == 0:
            return []
        st = self._stepper()
        n = self._n
        row = -1 if parentObjectUniqueId == -1 else int(parentLinkIndex) + 1
        hits = st.ray_test(np.concatenate([frm, to], axis=1), parent_row=row)[0].astype(np.float64)
        links = np.asarray(st.contact_links(), dtype=np.int64)
        out = []
        for r in hits:
            pid = int(r[7])
            body = int(self.segmentation_ids(pid))
            link = int(links[pid - 1]) if 1 <= pid <= 2 * n else -1
            out.append((body, link, float(r[0]), tuple(float(v) for v in r[1:4]), tuple(float(v) for v in r[4:7])))
        return out

    def rayTest(self, rayFromPosition, rayToPosition, **kw):
        """PyBullet's rayTest: rayTestBatch of the one ray (a list of one tuple)."""
        if kw:
            raise NotImplementedError("BulletClient.rayTest: %s" % sorted(kw))
        return self.rayTestBatch([rayFromPosition], [rayToPosition])
