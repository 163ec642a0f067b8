"""Drop-in compatibility layer: lets the reference's training scripts and cfg files run against
the MI355X-native environment without Isaac Sim / ORBIT.

    import isaac_rover_orbit_amd.compat as compat
    compat.install()                      # before importing rover_envs.* / examples/02_train/train.py
    import rover_envs.envs.navigation.robots           # the reference's own registration module, unchanged
    env = gym.make("AAURoverEnv-v0", cfg=parse_env_cfg("AAURoverEnv-v0", num_envs=4096))   # -> HIP-backed RoverEnv

``install()`` (1) registers the ``omni.isaac.orbit`` / ``omni.isaac.orbit_tasks`` / ``omni.isaac.core`` / ``carb`` / ``pxr``
import namespace of ``orbit_shim`` unless the real packages are importable, (2) provides a minimal gymnasium-style
registry when ``gymnasium`` is not installed, and (3) redirects the entry point of the rover task ids to
``isaac_rover_orbit_amd.envs:RoverEnv`` -- the reference's ``RoverEnv.step`` is exactly the hot path being replaced.
"""
from __future__ import annotations

import importlib
import importlib.util
import sys
import types

ROVER_TASK_IDS = ("AAURoverEnv-v0",)
_installed = False


# ------------------------------------------------------------------------------------------------- gym registry
class _Spec:
    def __init__(self, id, entry_point, kwargs):
        self.id, self.entry_point, self.kwargs = id, entry_point, dict(kwargs or {})


def _capped_cubic_video_schedule(episode_id: int) -> bool:
    """gymnasium's default episode trigger: episodes 0, 1, 8, 27, ... up to 1000, then every 1000th."""
    if episode_id < 1000:
        return int(round(episode_id ** (1.0 / 3))) ** 3 == episode_id
    return episode_id % 1000 == 0


def _episode_ended(terminated, truncated) -> bool:
    """Whether the (first) episode ended in this step: a batched env's flags are tensors / arrays, env 0's episode counts."""
    def first(x):
        if hasattr(x, "reshape"):
            x = x.reshape(-1)
            return bool(x[0]) if len(x) else False
        return bool(x)
    return first(terminated) or first(truncated)


class _RecordVideo:
    """``gymnasium.wrappers.RecordVideo`` for the minimal registry (no gymnasium, no video encoder installed): the reference's
    ``video_record()`` (examples/02_train/train.py:73-97) wraps the env in it when ``--video`` is given.

    When a trigger fires (``step_trigger(global step)`` or ``episode_trigger(episode)``; gymnasium's capped cubic episode schedule when
    neither is given) it collects ``env.render()`` frames -- the frame of the state at the trigger, then one per step -- until it holds
    ``video_length`` of them (0: until the episode ends), and writes them to ``{video_folder}/{name_prefix}-step-{k}.npz`` (or
    ``-episode-{k}``) as ``frames`` (T, H, W, 3) uint8.  Every other attribute, and ``unwrapped``, is the env's."""

    def __init__(self, env, video_folder, episode_trigger=None, step_trigger=None, video_length=0, name_prefix="rl-video", **_):
        import os
        if getattr(env, "render_mode", None) != "rgb_array":
            raise ValueError(f"RecordVideo needs an env with render_mode='rgb_array' (got {getattr(env, 'render_mode', None)!r})")
        if episode_trigger is None and step_trigger is None:
            episode_trigger = _capped_cubic_video_schedule
        self.env = env
        self.video_folder = os.path.abspath(video_folder)
        os.makedirs(self.video_folder, exist_ok=True)
        self.episode_trigger, self.step_trigger = episode_trigger, step_trigger
        self.video_length, self.name_prefix = int(video_length), name_prefix
        self.step_id = self.episode_id = 0
        self.recording, self.frames, self.video_name = False, [], None
        self.written = []                                  # paths of the npz files written so far

    def __getattr__(self, name):
        if name.startswith("__") or name == "env":
            raise AttributeError(name)
        return getattr(self.env, name)

    @property
    def unwrapped(self):
        return self.env.unwrapped

    def _triggered(self) -> bool:
        if self.step_trigger is not None:
            return bool(self.step_trigger(self.step_id))
        return bool(self.episode_trigger(self.episode_id))

    def _start(self):
        self.recording, self.frames = True, []
        self.video_name = (f"{self.name_prefix}-step-{self.step_id}" if self.step_trigger is not None
                           else f"{self.name_prefix}-episode-{self.episode_id}")
        self._capture()

    def _capture(self):
        import numpy as np
        self.frames.append(np.ascontiguousarray(self.env.render(), dtype=np.uint8))
        if self.video_length > 0 and len(self.frames) >= self.video_length:
            self._write()

    def _write(self):
        import os
        import numpy as np
        if self.recording and self.frames:
            path = os.path.join(self.video_folder, self.video_name + ".npz")
            np.savez(path, frames=np.stack(self.frames))
            self.written.append(path)
        self.recording, self.frames = False, []

    def reset(self, **kwargs):
        out = self.env.reset(**kwargs)
        if not self.recording and self._triggered():
            self._start()
        return out

    def step(self, action):
        out = self.env.step(action)
        self.step_id += 1
        ended = _episode_ended(out[2], out[3])
        if ended:
            self.episode_id += 1
        if self.recording:
            self._capture()
            if self.recording and self.video_length == 0 and ended:
                self._write()
        elif self._triggered():
            self._start()
        return out

    def close(self):
        self._write()
        return self.env.close()


class _MiniGym(types.ModuleType):
    """The three calls the reference makes on ``gymnasium``: register / make / spec (+ spaces.Box), and
    ``wrappers.RecordVideo`` for its ``--video`` flag."""

    def __init__(self, name="gymnasium"):
        super().__init__(name)
        self.registry = {}
        from ..envs.rover_env import _spaces
        self.spaces = types.ModuleType(name + ".spaces")
        self.spaces.Box = _spaces.Box
        self.spaces.Dict = _spaces.Dict
        self.spaces.__path__ = []
        self.spaces.box = types.ModuleType(name + ".spaces.box")
        self.spaces.box.Box = _spaces.Box
        self.Env = object
        self.wrappers = types.ModuleType(name + ".wrappers")
        self.wrappers.RecordVideo = _RecordVideo
        self.__path__ = []

    def register(self, id, entry_point=None, disable_env_checker=True, kwargs=None, **_):
        self.registry[id] = _Spec(id, entry_point, kwargs)

    def spec(self, id):
        return self.registry[id]

    def make(self, id, **kwargs):
        spec = self.registry[id]
        entry = spec.entry_point
        if isinstance(entry, str):
            mod, attr = entry.split(":")
            entry = getattr(importlib.import_module(mod), attr)
        kw = {k: v for k, v in spec.kwargs.items() if k not in ("env_cfg_entry_point", "best_model_path", "get_agent_fn")}
        kw.update(kwargs)
        return entry(**kw)


_gym = None


def gym_api():
    """gymnasium if installed, else the minimal registry above (shared singleton, also aliased as ``gym``)."""
    global _gym
    if _gym is None:
        try:
            import gymnasium
            _gym = gymnasium
        except ImportError:
            _gym = _MiniGym()
            sys.modules.setdefault("gymnasium", _gym)
            sys.modules.setdefault("gymnasium.spaces", _gym.spaces)
            sys.modules.setdefault("gymnasium.spaces.box", _gym.spaces.box)
            sys.modules.setdefault("gymnasium.wrappers", _gym.wrappers)
    return _gym


def _redirect_entry_points(gym):
    """Route the rover task ids to the HIP-backed env whenever they get registered (now or later)."""
    target = "isaac_rover_orbit_amd.envs:RoverEnv"
    orig_register = gym.register

    def register(id, entry_point=None, **kw):
        if id in ROVER_TASK_IDS:
            entry_point = target
        return orig_register(id, entry_point=entry_point, **kw)

    if not getattr(gym.register, "_rover_redirect", False):
        register._rover_redirect = True
        gym.register = register
    reg = getattr(gym, "registry", None)
    if isinstance(reg, dict):
        for tid in ROVER_TASK_IDS:
            if tid in reg and hasattr(reg[tid], "entry_point"):
                try:
                    reg[tid].entry_point = target
                except Exception:
                    pass


def install(force: bool = False) -> dict:
    """Install the compatibility namespace; returns {module name: module} of what was registered."""
    global _installed
    from . import orbit_shim
    registered = {}
    have_real_orbit = False
    if not force:
        try:
            have_real_orbit = importlib.util.find_spec("omni.isaac.orbit") is not None
        except (ImportError, ValueError):
            have_real_orbit = False
    if not have_real_orbit:
        for name, mod in orbit_shim.build_modules().items():
            if force or name not in sys.modules:
                sys.modules[name] = mod
                registered[name] = mod
    # pymeshlab is only touched by TerrainManager.get_mesh (USD mesh read-out, terrain_utils.py:129-155), which this
    # path replaces by isaac_rover_orbit_amd.terrain; let the import of terrain_utils succeed without it
    try:
        have_pymeshlab = importlib.util.find_spec("pymeshlab") is not None
    except (ImportError, ValueError):
        have_pymeshlab = False
    if not have_pymeshlab and "pymeshlab" not in sys.modules:
        stub = types.ModuleType("pymeshlab")

        def _no_pymeshlab(*a, **k):
            raise RuntimeError("pymeshlab is not installed; use isaac_rover_orbit_amd.terrain.terrain_from_mesh instead")
        stub.Mesh = stub.MeshSet = _no_pymeshlab
        sys.modules["pymeshlab"] = stub
        registered["pymeshlab"] = stub
    gym = gym_api()
    if "gym" not in sys.modules:            # the reference's learning glue still imports the legacy name (`from gym.spaces import Box`)
        sys.modules["gym"] = gym
        sys.modules["gym.spaces"] = gym.spaces
        if hasattr(gym.spaces, "box"):
            sys.modules["gym.spaces.box"] = gym.spaces.box
    _redirect_entry_points(gym)
    _installed = True
    return registered


def register_default_tasks():
    """Register ``AAURoverEnv-v0`` and ``RoverCamera-v0`` with this package's own cfg (for users who do not have the reference
    checked out)."""
    from ..cfg import AAURoverCameraEnvCfg, AAURoverEnvCfg
    gym = gym_api()
    gym.register(id="AAURoverEnv-v0", entry_point="isaac_rover_orbit_amd.envs:RoverEnv", disable_env_checker=True,
                 kwargs={"env_cfg_entry_point": AAURoverEnvCfg})
    # rover_envs/envs/__init__.py:38-42 reserves the id (registration commented out there); entry point rover_camera_env.py:18
    gym.register(id="RoverCamera-v0", entry_point="isaac_rover_orbit_amd.envs:RoverEnvCamera", disable_env_checker=True,
                 kwargs={"env_cfg_entry_point": AAURoverCameraEnvCfg})
    from ..envs.lift_env import LiftEnvCfg
    # manipulation/config/franka/__init__.py:6-14 (entry point there: ORBIT's generic RLTaskEnv on FrankaCubeLiftEnvCfg)
    gym.register(id="FrankaCubeLift-v0", entry_point="isaac_rover_orbit_amd.envs:FrankaCubeLiftEnv", disable_env_checker=True,
                 kwargs={"env_cfg_entry_point": LiftEnvCfg})
