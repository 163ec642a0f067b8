"""Translate a reference-style cfg object (an instance of the reference's ``AAURoverEnvCfg`` built on ORBIT -- or on
``compat.orbit_shim`` -- configclasses) into this package's ``RoverEnvCfg`` / kernel parameter block.

Field map (reference file:line -> here):
  scene.num_envs                                   rover_env_cfg.py:233-234      -> scene.num_envs
  sim.dt / decimation / episode_length_s           rover_env_cfg.py:269-271      -> sim.dt / decimation / episode_length_s
  actions.actions (AckermannActionCfg)             aau_rover/env_cfg.py:21-31    -> actions.*
  observations.policy.<term>.scale / noise / clip  rover_env_cfg.py:97-123       -> observations[...].scale / .noise / .clip
  rewards.<term>.weight / params                   rover_env_cfg.py:126-163      -> rewards[...]
  terminations.<term>.params / time_out            rover_env_cfg.py:166-183      -> terminations[...]
  commands.target_pose.*                           rover_env_cfg.py:187-200      -> commands.*
  scene.height_scanner.pattern_cfg / offset        rover_env_cfg.py:78-86        -> height_scanner.*
Built-in term functions are matched by table key and ``func.__name__``.  A reward / termination entry under another key
is a USER-WRITTEN term (the reference's tables hold arbitrary ``func=``, rover_env_cfg.py:126-183): its callable and params
are kept as they are (``SceneEntityCfg`` objects included) and ``RoverEnv.step`` evaluates it in torch between the two halves
of the step (the slow path).  A built-in reward that the cfg omits is switched off (weight 0); an omitted ``is_success`` /
``far_from_target`` termination gets a threshold no distance can meet -- the REWARD term of the same name keeps its own threshold
(``rover_config.rew_success_threshold`` / ``rew_far_threshold``: rover_env_cfg.py:136,162 vs :173,177 are independent entries);
``time_limit`` and ``collision`` cannot be omitted.
``log_values`` of a converted cfg is ``"host"`` (the reference trainer's per-step ``.item()`` reads, skrl_utils.py:139-142).
"""
from __future__ import annotations

from ..cfg import OBS_ORDER, REWARD_FUNCS, REWARD_ORDER, TERMINATION_FUNCS, TERMINATION_ORDER, RoverEnvCfg, TermCfg, ViewerCfg


def is_reference_cfg(cfg) -> bool:
    return hasattr(cfg, "scene") and hasattr(cfg, "rewards") and not isinstance(getattr(cfg, "rewards"), dict)


def _func_name(f):
    return f if isinstance(f, str) else getattr(f, "__name__", str(f))


def _plain_params(params):
    out = {}
    for k, v in (params or {}).items():
        out[k] = getattr(v, "name", v) if v.__class__.__name__ == "SceneEntityCfg" else v
    return out


def _terms(table, order, what, allow_custom=False):
    found = {k: v for k, v in vars(table).items() if hasattr(v, "func")}
    if not allow_custom and list(found) != order:
        raise ValueError(f"{what} terms of the cfg are {list(found)}; the fused kernels implement exactly {order}")
    return found


def from_reference_cfg(ref) -> RoverEnvCfg:
    out = RoverEnvCfg()
    out.scene.num_envs = int(ref.scene.num_envs)
    out.scene.env_spacing = getattr(ref.scene, "env_spacing", out.scene.env_spacing)
    out.sim.dt = float(ref.sim.dt)
    dev = getattr(ref.sim, "device", None)
    if dev:
        out.sim.device = dev
    out.decimation = int(ref.decimation)
    out.episode_length_s = float(ref.episode_length_s)

    act = ref.actions.actions
    a = out.actions
    a.scale, a.offset = tuple(act.scale), act.offset
    a.wheelbase_length, a.middle_wheel_distance = act.wheelbase_length, act.middle_wheel_distance
    a.rear_and_front_wheel_distance, a.wheel_radius = act.rear_and_front_wheel_distance, act.wheel_radius
    a.min_steering_radius = act.min_steering_radius

    obs = _terms(ref.observations.policy, OBS_ORDER, "observation")
    corrupt = bool(getattr(ref.observations.policy, "enable_corruption", False))   # ObservationManager: noise only if the group says so
    for name, t in obs.items():
        clip = getattr(t, "clip", None)
        out.observations[name] = TermCfg(_func_name(t.func), scale=1.0 if t.scale is None else float(t.scale),
                                         params=_plain_params(t.params), noise=getattr(t, "noise", None) if corrupt else None,
                                         clip=None if clip is None else (float(clip[0]), float(clip[1])))
    rew = _terms(ref.rewards, REWARD_ORDER, "reward", allow_custom=True)
    for name, fn in zip(REWARD_ORDER, REWARD_FUNCS):
        if name in rew:
            if _func_name(rew[name].func) != fn:
                raise ValueError(f"reward term '{name}' is a built-in name and must use '{fn}' (got '{_func_name(rew[name].func)}'); "
                                 "give a user-written term another key")
            out.rewards[name] = TermCfg(fn, weight=float(rew[name].weight), params=_plain_params(rew[name].params))
        else:
            out.rewards[name].weight = 0.0            # omitted by the user's table: the kernel term stays, switched off
    for name, t in rew.items():
        if name not in REWARD_ORDER:
            if not callable(t.func):
                raise ValueError(f"reward term '{name}': func is not callable")
            out.rewards[name] = TermCfg(t.func, weight=float(t.weight), params=dict(t.params or {}))
    ter = _terms(ref.terminations, TERMINATION_ORDER, "termination", allow_custom=True)
    for name, fn in zip(TERMINATION_ORDER, TERMINATION_FUNCS):
        if name in ter:
            if _func_name(ter[name].func) != fn:
                raise ValueError(f"termination term '{name}' is a built-in name and must use '{fn}' (got '{_func_name(ter[name].func)}')")
            out.terminations[name] = TermCfg(fn, params=_plain_params(ter[name].params), time_out=bool(ter[name].time_out))
        elif name == "is_success":
            out.terminations[name].params["threshold"] = -1.0           # d < -1 never holds; the reached_target REWARD keeps its own
        elif name == "far_from_target":                                 # threshold (rover_env_cfg.py:136 / :162 are entries of their own)
            out.terminations[name].params["threshold"] = float("inf")   # d > inf never holds
        else:
            raise ValueError(f"the built-in termination '{name}' cannot be omitted (the episode clock / the contact report end episodes in the kernel)")
    for name, t in ter.items():
        if name not in TERMINATION_ORDER:
            if not callable(t.func):
                raise ValueError(f"termination term '{name}': func is not callable")
            out.terminations[name] = TermCfg(t.func, params=dict(t.params or {}), time_out=bool(getattr(t, "time_out", False)))

    cmd = ref.commands.target_pose
    out.commands.resampling_time_range = tuple(cmd.resampling_time_range)
    out.commands.heading_range = tuple(cmd.ranges.heading)
    out.commands.simple_heading = bool(cmd.simple_heading)

    hs = ref.scene.height_scanner
    out.height_scanner.resolution = float(hs.pattern_cfg.resolution)
    out.height_scanner.size = tuple(hs.pattern_cfg.size)
    out.height_scanner.offset_z = float(hs.offset.pos[2])
    out.height_scanner.attach_yaw_only = bool(hs.attach_yaw_only)
    out.height_scanner.max_distance = float(hs.max_distance)
    if not out.height_scanner.attach_yaw_only:
        raise ValueError("attach_yaw_only=False is not supported (the reference cfg uses True, rover_env_cfg.py:81)")
    rnd = getattr(ref, "randomization", None)
    if rnd is not None and hasattr(rnd, "reset_state"):
        out.reset_z_offset = float(rnd.reset_state.params.get("z_offset", 0.5))
    # The consumer of a converted cfg is the reference's own trainer stack, which calls .item() on every entry of infos["episode"]
    # after EVERY step (rover_envs/utils/skrl_utils.py:139-142): with 0-d DEVICE tensors that is thirteen host synchronisations per
    # step (~290 us), with the pinned host mirror one copy and one synchronisation (~100 us) -- same numbers, and 0-d CPU tensors
    # satisfy the isinstance / numel() checks of that loop.  The native RoverEnvCfg keeps ORBIT's "device".
    out.log_values = "host"
    vw = getattr(ref, "viewer", None)
    if vw is not None:
        out.viewer = viewer_from_reference(vw)
    out.validate()
    return out


def viewer_from_reference(vw) -> ViewerCfg:
    """ORBIT's ``cfg.viewer`` (eye, lookat, resolution; rover_env_cfg.py:272 sets the eye) as the rgb_array viewer's cfg."""
    out = ViewerCfg()
    out.eye = tuple(float(x) for x in vw.eye)
    out.lookat = tuple(float(x) for x in getattr(vw, "lookat", out.lookat))
    out.resolution = tuple(int(x) for x in getattr(vw, "resolution", out.resolution))
    return out
