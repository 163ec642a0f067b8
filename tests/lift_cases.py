"""Cases of the FrankaCubeLift-v0 step off its defaults, shared by the CPU tests (tests/test_lift_oracle.py: the oracle alone
reaches every branch the GPU tests rely on) and the GPU tests (tests/test_gpu_lift_edges.py: the HIP step against the oracle on
the same inputs, bit for bit).

A case is a dictionary of ``lift_config`` fields (include/rover_lift.h) laid over the defaults, a batch size and a run length.
``CaseCfg`` carries it into ``FrankaCubeLiftEnv``: a ``LiftEnvCfg`` whose ``to_native()`` is the case's struct, so that the fields
``LiftEnvCfg`` has no attribute for (``mu_table``, ``mu_pad``) and ``decimation = 0`` are reachable.  ``stagger`` spreads the
episode counters, the command timers and a few dropped cubes over the envs, so that the lanes of one wave take different sides
of the reset and resample selects in the same step.  ``oracle_run`` is the reference trajectory, computed once per case."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

LANES = 8                      # envs per wave of the product form (eight lanes per env)
PRODUCT, SINGLE, SHADOWED = (8, True), (8, False), (16, False)       # (lanes per env, pipelined): rover_lift_debug_set_*
FORMS = {"product": PRODUCT, "single": SINGLE, "shadowed": SHADOWED}


def episode(steps: int, sim_dt: float = 0.01, decimation: int = 2) -> dict:
    """The three fields of an episode of ``steps`` env steps (``decimation = 0``: the length in seconds is the log's divisor only)."""
    step_dt = sim_dt * decimation
    return {"sim_dt": sim_dt, "decimation": decimation, "max_episode_length": steps,
            "max_episode_length_s": steps * step_dt if decimation > 0 else 0.8}


@dataclass
class Case:
    name: str
    over: dict                        # lift_config fields laid over the defaults
    n: int = 37
    steps: int = 60
    forms: tuple = ("product",)
    seed: int = 0                     # of the actions


NAMED = [
    # the staggered case: default physics, the timer fires about every fifteenth step
    Case("stagger", {"cmd_resample_time": 0.3}),
    # decimation: no substep at all, the single-substep form, both parities of the pipelined hand buffer beyond two substeps
    Case("decimation0", {**episode(40, decimation=0), "cmd_resample_time": 0.3, "action_scale": 1.5}, n=13, forms=tuple(FORMS)),
    Case("decimation1", {**episode(50, decimation=1), "solver_iterations": 3, "cmd_resample_time": 0.1}, n=21, steps=80,
         forms=tuple(FORMS)),
    Case("decimation3", {**episode(40, decimation=3), "solver_iterations": 1, "cmd_resample_time": 0.3}, n=29, forms=tuple(FORMS)),
    Case("decimation4_dt", {**episode(50, sim_dt=0.005, decimation=4), "cmd_resample_time": 0.3}, n=15, steps=80,
         forms=tuple(FORMS)),
    # no solver sweep: the cube sinks through the table, drops without injection
    Case("no_sweeps", {**episode(45), "solver_iterations": 0, "cmd_resample_time": 0.3}, n=33, steps=100, forms=tuple(FORMS)),
    Case("actuation", {**episode(35), "action_scale": 1.5, "finger_open": 0.03, "finger_close": 0.01, "ee_offset_z": 0.12,
                       "mu_table": 0.05, "mu_pad": 2.0, "cmd_resample_time": 0.3}, n=23),
    Case("rewards", {**episode(30), "rew_weight": (0.0, 15.0, -16.0, 5.0, 0.0, 1.0e-4), "reach_std": 0.25, "goal_std": 0.5,
                     "goal_fine_std": 0.02, "minimal_height": 0.03, "drop_height": 0.02, "cmd_resample_time": 0.3}, n=19),
    Case("commands", {**episode(25), "cmd_lo": (0.35, 0.5, 0.1), "cmd_hi": (0.65, 0.5, 0.4), "cmd_resample_time": 0.02,
                      "obj_init": (0.45, 0.1, 0.08), "obj_range_lo": (-0.05, -0.1, 0.0), "obj_range_hi": (0.15, 0.2, 0.05),
                      "seed_lo": 12345, "seed_hi": 0x9E3779B9}, n=27, steps=40),
    Case("reset_every_step", {**episode(1), "max_episode_length_s": 5.0, "cmd_resample_time": 0.02, "seed_hi": 7}, n=11, steps=40),
]


def random_case(seed: int) -> Case:
    """Every field of ``lift_config`` drawn at once (the rover's test_random_configurations_match_oracle, for the lift task)."""
    rng = np.random.RandomState(200 + seed)
    decimation = int(rng.choice([1, 2, 3, 4]))
    sim_dt = float(rng.choice([0.005, 0.01, 0.0125]))
    over = episode(int(rng.randint(5, 60)), sim_dt, decimation)
    over["solver_iterations"] = int(rng.randint(0, 10))
    over["action_scale"] = float(rng.uniform(0.2, 1.5))
    over["finger_open"], over["finger_close"] = float(rng.uniform(0.025, 0.04)), float(rng.uniform(0.0, 0.015))
    over["ee_offset_z"] = float(rng.uniform(0.09, 0.13))
    over["mu_table"], over["mu_pad"] = float(rng.uniform(0.05, 1.0)), float(rng.uniform(0.3, 2.0))
    default_w = np.array([1.0, 15.0, 16.0, 5.0, 1.0e-3, 1.0e-4])
    over["rew_weight"] = tuple(float(w) for w in default_w * rng.uniform(-1.0, 2.0, 6) * (rng.uniform(0, 1, 6) > 0.25))
    over["reach_std"], over["goal_std"], over["goal_fine_std"] = (float(rng.uniform(*r)) for r in ((0.05, 0.3), (0.1, 0.6), (0.02, 0.1)))
    over["minimal_height"] = float(rng.uniform(0.02, 0.08))
    over["drop_height"] = float(rng.choice([-0.05, 0.0, 0.02]))
    lo = rng.uniform([0.3, -0.3, 0.0], [0.5, 0.3, 0.2])
    width = rng.uniform(0.0, 0.4, 3) * (rng.uniform(0, 1, 3) > 0.3)             # some axes with lo == hi
    over["cmd_lo"], over["cmd_hi"] = tuple(float(v) for v in lo), tuple(float(v) for v in lo + width)
    over["cmd_resample_time"] = float(rng.choice([0.02, 0.1, 0.3, 5.0]))
    over["obj_init"] = tuple(float(v) for v in rng.uniform([0.4, -0.1, 0.03], [0.6, 0.1, 0.1]))
    rlo = rng.uniform([-0.15, -0.25, 0.0], [0.0, 0.0, 0.0])
    over["obj_range_lo"], over["obj_range_hi"] = tuple(float(v) for v in rlo), tuple(float(v) for v in rlo + rng.uniform(0.0, 0.3, 3))
    over["seed_lo"], over["seed_hi"] = int(rng.randint(0, 2 ** 31)), int(rng.randint(0, 2 ** 31))
    return Case(f"random{seed}", over, n=int(rng.randint(7, 38)), steps=60, seed=seed)


RANDOM = [random_case(s) for s in range(6)]
CASES = NAMED + RANDOM
BY_NAME = {c.name: c for c in CASES}
CONFIG_FIELDS = ("sim_dt", "decimation", "max_episode_length", "max_episode_length_s", "action_scale", "finger_open", "finger_close",
                 "rew_weight", "reach_std", "goal_std", "goal_fine_std", "minimal_height", "drop_height", "cmd_lo", "cmd_hi",
                 "cmd_resample_time", "obj_init", "obj_range_lo", "obj_range_hi", "ee_offset_z", "seed_lo", "seed_hi",
                 "solver_iterations", "mu_table", "mu_pad")


def apply_over(c, over: dict):
    """Lay ``over`` on a ctypes config struct (the oracle's or the library's: the same fields in the same order)."""
    for k, v in over.items():
        if isinstance(v, (list, tuple, np.ndarray)):
            for i, x in enumerate(v):
                getattr(c, k)[i] = x
        else:
            setattr(c, k, v)
    return c


def oracle_config(lo, over: dict):
    return apply_over(lo.default_config(), over)


def make_env(over: dict, n: int, env_id_offset: int = 0, log_reduction: str = "on_demand", form=None):
    """``FrankaCubeLiftEnv`` on the case's struct (needs the GPU).  ``form``: (lanes per env, pipelined) through the two debug
    setters, None = what the library chooses."""
    import ctypes as C

    from isaac_rover_orbit_amd import _lib
    from isaac_rover_orbit_amd.envs import FrankaCubeLiftEnv, LiftEnvCfg

    @dataclass
    class CaseCfg(LiftEnvCfg):
        native_over: dict = field(default_factory=dict)

        @property
        def max_episode_length(self) -> int:
            return int(self.to_native().max_episode_length)

        def to_native(self):
            c = _lib.LiftConfig()
            _lib.check(_lib.load().rover_lift_default_config(C.byref(c)), "rover_lift_default_config")
            return apply_over(c, self.native_over)

    cfg = CaseCfg(native_over=dict(over))
    cfg.scene.num_envs, cfg.env_id_offset, cfg.log_reduction = n, env_id_offset, log_reduction
    native = cfg.to_native()
    cfg.sim.dt, cfg.decimation, cfg.ee_offset_z = native.sim_dt, native.decimation, native.ee_offset_z
    cfg.seed = native.seed_lo | (native.seed_hi << 32)
    env = FrankaCubeLiftEnv(cfg)
    if form is not None:
        lanes, pipe = form
        assert env._lib.rover_lift_debug_set_lanes(env._h, lanes) == 0 and env._lib.rover_lift_debug_set_pipeline(env._h, int(pipe)) == 0
        assert env.kernel_name() == f"lift_step_kernel<{lanes}, {'true' if pipe else 'false'}>"
    return env


def stagger(lo, cfg, S: np.ndarray) -> np.ndarray:
    """Edit an oracle state (n, 64) in place: episode counters (37 e) mod the episode length, command timers 1 .. 15 steps from
    firing, the cube of every fifth env below any drop height."""
    n = S.shape[0]
    e = np.arange(n)
    S[:, lo.EP_LEN] = ((37 * e) % cfg.max_episode_length).astype(np.int32).view(np.float32)
    step_dt = np.float32(cfg.sim_dt) * np.float32(cfg.decimation)
    S[:, lo.TIME_LEFT] = step_dt * (1 + e % 15).astype(np.float32)
    S[0::5, lo.OBJ_POS + 2] = -0.2
    return S


def actions(rng, k: int, n: int) -> np.ndarray:
    a = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
    if k % 20 < 10:
        a[:, 7] = -1.0                     # the gripper closes half the time
    return a


@dataclass
class Run:
    cfg: object
    obs_reset: np.ndarray             # observations of reset()
    S_reset: np.ndarray               # state after reset()
    S0: np.ndarray                    # state the steps start from (staggered, or S_reset)
    steps: list                       # per step: dict(a, obs, rew, term, trunc, log, S, resampled)


_RUNS: dict = {}


def oracle_run(lo, over: dict, n: int, steps: int, seed: int = 0, env_id_offset: int = 0, staggered: bool = True, key=None) -> Run:
    """reset() and ``steps`` closed-loop steps of the oracle.  ``resampled``: the envs whose command timer fired in the step, read
    off the per-episode resample index (word 63: 0 after a reset, + 1 per timer resample).  Cached under ``key``; read only."""
    if key is not None and key in _RUNS:
        return _RUNS[key]
    cfg = oracle_config(lo, over)
    S = lo.new_state(n)
    obs_reset = lo.reset(cfg, S, env_id_offset)
    S_reset = S.copy()
    if staggered:
        stagger(lo, cfg, S)
    S0 = S.copy()
    rng = np.random.RandomState(seed)
    log = np.zeros(lo.LOG_WORDS, np.float32)
    out = []
    for k in range(steps):
        a = actions(rng, k, n)
        before = S[:, lo.CMD_COUNT].view(np.uint32).copy()
        obs, rew, term, trunc, log = lo.step(cfg, S, a, env_id_offset, log=log)
        reset = (term | trunc).astype(bool)
        after = S[:, lo.CMD_COUNT].view(np.uint32)
        resampled = np.where(reset, after == 1, after == before + 1)
        assert (np.where(reset, after <= 1, (after == before) | resampled)).all()
        out.append(dict(a=a, obs=obs, rew=rew, term=term.astype(bool), trunc=trunc.astype(bool), log=log.copy(), S=S.copy(),
                        resampled=resampled))
    run = Run(cfg, obs_reset, S_reset, S0, out)
    if key is not None:
        _RUNS[key] = run
    return run


def case_run(lo, case: Case) -> Run:
    return oracle_run(lo, case.over, case.n, case.steps, case.seed, key=("case", case.name))


def _mixed(flags: np.ndarray) -> int:
    """Waves of eight envs (the last one partly filled: its spare lanes repeat the last env) in which some but not all flags are set."""
    count = 0
    for w in range(0, flags.shape[0], LANES):
        f = flags[w:w + LANES]
        count += int(f.any() and not f.all())
    return count


def reach_counts(run: Run) -> dict:
    """How often a run does what the default configuration never does (the GPU tests must not pass by never getting there)."""
    c = dict(drops=0, time_outs=0, resamples=0, resample_with_reset=0, mixed_reset_waves=0, mixed_resample_waves=0,
             drop_and_time_out_steps=0)
    for s in run.steps:
        reset = s["term"] | s["trunc"]
        c["drops"] += int(s["term"].sum())
        c["time_outs"] += int(s["trunc"].sum())
        c["resamples"] += int(s["resampled"].sum())
        c["resample_with_reset"] += int((s["resampled"] & reset).sum())
        c["mixed_reset_waves"] += _mixed(reset)
        c["mixed_resample_waves"] += _mixed(s["resampled"])
        c["drop_and_time_out_steps"] += int((s["term"] & ~s["trunc"]).any() and (s["trunc"] & ~s["term"]).any())
    return c


def moved_fields(lo) -> set:
    """The ``lift_config`` fields some case moves off the default."""
    default = lo.default_config()
    moved = set()
    for case in CASES:
        c = oracle_config(lo, case.over)
        for name in CONFIG_FIELDS:
            a, b = getattr(default, name), getattr(c, name)
            if (list(a) != list(b)) if hasattr(a, "__len__") else (a != b):
                moved.add(name)
    return moved


def by_hand_command(cfg, gid, count, index):
    """The command position ``resample_command`` draws at Philox counter (gid, count, 1, index), from the package's numpy Philox:
    uniform = (word >> 8) * 2**-24, position = lo + uniform * (hi - lo) with hi - lo in float32.  The product is exact in float64
    and the sum is rounded twice (float64, then float32) where the kernel's fma rounds once: within 1 ulp."""
    from isaac_rover_orbit_amd.rollout import philox4x32
    r = philox4x32(gid, count, 1, index, cfg.seed_lo, cfg.seed_hi)
    out = []
    for k in range(3):
        u = (np.asarray(r[k], np.uint64) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        lo_k, d = np.float32(cfg.cmd_lo[k]), np.float32(cfg.cmd_hi[k]) - np.float32(cfg.cmd_lo[k])
        out.append((u * np.float64(d) + np.float64(lo_k)).astype(np.float32))
    return np.stack(out, axis=-1)
