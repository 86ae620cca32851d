"""bullet-envs_amd -- MI355X-native batched stepper for the SnakeGymEnv step/reset path.

The directory name carries the reference's hyphen, so import it through importlib
    pkg = importlib.import_module("bullet-envs_amd")
or through the top-level shim:  import bullet_envs_amd as pkg
"""
from ._lib import SnkParams, Snapshot, Stepper, default_params, load, LIB_PATH, trace_row_floats, trace_to_lists  # noqa: F401
from ._lib import PAIRS_BOX, PAIRS_LINKS  # noqa: F401  (flags of closest_points)
from ._lib import RAYS_ALL, RAYS_BOX, RAYS_GROUND, RAYS_SNAKE  # noqa: F401  (flags of ray_test)
from .snake_env import (CloudpickleWrapper, Snake, SnakeGymEnv, SnakeVecEnv, SubprocVecEnv, VecEnv,  # noqa: F401
                        params_from_args)
from .device_env import DeviceVecEnv, DeviceWorld, ShardedVecEnv  # noqa: F401
from .pybullet_client import BulletClient  # noqa: F401  (the reference's inner seam: Snake(pybullet_client, ...))
from . import checkpoint  # noqa: F401  (simulator-state checkpoints)
from .checkpoint import save_state, load_state  # noqa: F401
try:        # the trainer-side pieces need torch; the env itself does not
    from . import rollout  # noqa: F401  (on-device policy inference / rollout buffer)
    from . import ars  # noqa: F401      (ARS normaliser + linear policies on device)
except ImportError:  # pragma: no cover
    rollout = ars = None
