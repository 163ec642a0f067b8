"""FrankaCubeLift-v0 off its defaults on the MI355X: the HIP step (csrc/lift_kernels.hip) against the scalar CPU oracle
(oracle/lift_oracle.c) on the same inputs, under the rule of tests/test_gpu_lift.py -- state, observations, rewards, terminated
and truncated bit for bit at every step, extras["log"][:8] to rtol 1e-5 (atol 1e-7), [8] exactly.  The cases are those of
tests/lift_cases.py; tests/test_lift_oracle.py shows with the oracle alone that they reach drops, time-outs, timer resamples of
the command (also in the step of a reset), waves whose eight envs take different sides of the reset and resample selects, and
every field of lift_config."""
import ctypes as C

import numpy as np
import pytest
import torch

import lift_cases as LC
from helpers import assert_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lo():
    from oracle import lift_oracle
    lift_oracle.build()
    lift_oracle.lib()
    return lift_oracle


def bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).view(np.int32)


def same_bits(got, want, what):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} words differ, first at {tuple(bad[0])}"


def read_log(env, info):
    """extras["log"] as the 9-vector of the oracle: a read of the dictionary reduces (on demand) or finds the step's reduction."""
    return np.array([float(v) for v in info["log"].values()] + [float(env._log[8])], np.float32)


def check_log(log, want, what):
    assert log[8] == want[8], (what, log[8], want[8])
    assert_close(log[:8], want[:8], 1e-7, 1e-5, what)


def check_config(lo, env, run):
    """The env runs on the struct the oracle ran on, byte for byte."""
    assert C.sizeof(env._native_cfg) == C.sizeof(run.cfg) and bytes(env._native_cfg) == bytes(run.cfg)


def follow(env, run, what, rows=slice(None), check_the_log=True):
    """reset() and the run's steps on ``env`` against the oracle's trajectory (``rows``: the shard of it this env holds)."""
    obs, _ = env.reset()
    same_bits(obs["policy"], run.obs_reset[rows], f"{what}: obs after reset")
    same_bits(env.get_state(), run.S_reset[rows], f"{what}: state after reset")
    env.set_state(torch.from_numpy(run.S0[rows]))
    for k, s in enumerate(run.steps):
        obs, rew, term, trunc, info = env.step(torch.from_numpy(s["a"][rows]).to(env.device))
        assert np.array_equal(term.cpu().numpy(), s["term"][rows]) and np.array_equal(trunc.cpu().numpy(), s["trunc"][rows]), (what, k)
        same_bits(obs["policy"], s["obs"][rows], f"{what}: obs step {k}")
        same_bits(rew, s["rew"][rows], f"{what}: reward step {k}")
        same_bits(env.get_state(), s["S"][rows], f"{what}: state step {k}")
        if check_the_log:
            check_log(read_log(env, info), s["log"], f"{what}: log step {k}")


@pytest.mark.parametrize("name,form", [(c.name, f) for c in LC.CASES for f in c.forms])
def test_lift_configurations_match_oracle(lo, name, form):
    """Every named and random configuration from the staggered state, random actions with the gripper closing half the time; the
    product form (two pipelined waves per eight envs), and for the decimation and solver-iteration cases the single-wave and the
    shadowed sixteen-lane forms as well."""
    case = LC.BY_NAME[name]
    run = LC.case_run(lo, case)
    env = LC.make_env(case.over, case.n, form=LC.FORMS[form])
    check_config(lo, env, run)
    follow(env, run, f"{name}/{form}")
    env.close()


@pytest.mark.parametrize("mode,every", [("every_step", 1), ("on_demand", 1), ("on_demand", 3), ("on_demand", 7)])
@pytest.mark.parametrize("episode_steps", [250, 12])
def test_lift_log_cadences_on_staggered_resets(lo, episode_steps, mode, every):
    """The staggered case (250-step episodes: a few steps with resets, long stretches without) and its twin with 12-step episodes
    (two to ten envs reset in EVERY step, so log rows tagged with different launch serials always lie side by side).  Reduced
    behind every step, or on demand after every step / every third / every seventh: at each read the vector is what the
    oracle's per-step reduction holds there, [8] = 0 included when the latest resets are older than the latest step.  A second
    flush without a step in between reports [8] = 0 and leaves [0..7] alone."""
    case = LC.BY_NAME["stagger"]
    over = case.over if episode_steps == 250 else {**case.over, **LC.episode(episode_steps)}
    run = LC.oracle_run(lo, over, case.n, case.steps, case.seed, key=("log", episode_steps))
    env = LC.make_env(over, case.n, log_reduction=mode, form=LC.PRODUCT)
    check_config(lo, env, run)
    env.reset()
    env.set_state(torch.from_numpy(run.S0))
    reads = stale = fresh = 0
    for k, s in enumerate(run.steps):
        obs, rew, term, trunc, info = env.step(torch.from_numpy(s["a"]).to(env.device))
        same_bits(obs["policy"], s["obs"], f"obs step {k}")
        if k % every != every - 1:
            continue
        log = env._log.cpu().numpy().copy() if mode == "every_step" else read_log(env, info)
        check_log(log, s["log"], f"{mode}/{every}: log step {k}")
        reads += 1
        fresh += int(s["log"][8] > 0)
        stale += int(s["log"][8] == 0 and s["log"][:8].any())
        if mode == "on_demand":
            env._log_pending = True                   # force the second flush: the dictionary itself flushes once per step
            env.flush_log()
            again = env._log.cpu().numpy()
            assert again[8] == 0 and np.array_equal(again[:8].view(np.int32), log[:8].view(np.int32)), k
    assert reads == len(run.steps) // every and (stale >= 2 if episode_steps == 250 else fresh == reads), (reads, fresh, stale)
    env.close()


@pytest.mark.parametrize("n,form", [(1, "product"), (1, "single"), (1, "shadowed"), (7, "product"), (9, "product")])
def test_lift_partly_filled_waves(lo, n, form):
    """Fewer envs than a wave holds, and one more than it holds: the spare lanes recompute the last env and store nothing.
    60 staggered steps."""
    over = {"cmd_resample_time": 0.3, **LC.episode(20)}
    run = LC.oracle_run(lo, over, n, 60, seed=n, key=("small", n))
    assert sum(int(s["trunc"].sum()) for s in run.steps) >= 2 * n and sum(int(s["resampled"].sum()) for s in run.steps) >= 2 * n
    env = LC.make_env(over, n, form=LC.FORMS[form])
    follow(env, run, f"n={n}/{form}")
    env.close()


def test_lift_shards_equal_the_whole_gpu(lo):
    """17 envs at env_id_offset = 64 as one env and as 8 at 64 next to 9 at 72 (the CPU test's case): reset() and 40 staggered
    steps, every env against its rows of the oracle's whole."""
    over = {"cmd_resample_time": 0.3, "seed_lo": 9, **LC.episode(30)}
    whole = LC.oracle_run(lo, over, 17, 40, seed=4, env_id_offset=64, key=("shards", 17))
    for rows, offset in ((slice(0, 17), 64), (slice(0, 8), 64), (slice(8, 17), 72)):
        env = LC.make_env(over, rows.stop - rows.start, env_id_offset=offset, form=LC.PRODUCT)
        follow(env, whole, f"rows {rows.start}:{rows.stop} at {offset}", rows=rows, check_the_log=rows == slice(0, 17))
        env.close()


def test_lift_automatic_form_on_both_sides_of_its_boundary(lo):
    """The pipelined form is chosen while its two waves per eight envs all fit the chip's SIMDs at once: 4 x SIMDs envs run
    lift_step_kernel<8, true>, eight more lift_step_kernel<8, false>; both agree with the oracle for two steps after reset()."""
    simd = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    for n, name in ((4 * simd, "lift_step_kernel<8, true>"), (4 * simd + 8, "lift_step_kernel<8, false>")):
        run = LC.oracle_run(lo, {}, n, 2, seed=1, staggered=False)
        env = LC.make_env({}, n)
        assert env.kernel_name() == name, (n, env.kernel_name())
        follow(env, run, f"n={n}")
        assert env.kernel_name() == name
        env.close()


def test_lift_terms_under_moved_stds(lo, golden_dir):
    """rover_lift_terms reads the stds and the minimal height from the handle's configuration: moved, against the oracle's
    restatement with the same values, bit for bit (rows of the reference fixture: both sides of every threshold)."""
    g = np.load(f"{golden_dir}/lift_terms.npz")
    moved = dict(reach_std=0.25, goal_std=0.5, goal_fine_std=0.02, minimal_height=0.03)
    env = LC.make_env(moved, 8)
    args = g["object_pos_w"], g["ee_pos_w"], g["robot_root_state_w"], g["command"]
    got = [t.cpu().numpy() for t in env.terms(*args)]
    want = lo.terms(*args, **{k: float(np.float32(v)) for k, v in moved.items()})
    default = lo.terms(*args)
    for a, b, d, nm in zip(got, want, default, ("lifted", "reach", "goal", "fine", "pos_b")):
        same_bits(a, b, nm)
        assert nm == "pos_b" or not np.array_equal(b, d), f"{nm}: the moved values change nothing"
    env.close()


def test_lift_checkpoint_carries_the_resample_index(lo):
    """A checkpoint taken mid-episode at command_resampling_time = 0.3 s, loaded into an env created with another seed: it goes on
    with the same commands as the env it was taken from and as the oracle, so word 63 and the key travel with it."""
    over = {"cmd_resample_time": 0.3, "seed_lo": 21, "seed_hi": 5}
    n, taken_at = 13, 40
    run = LC.oracle_run(lo, over, n, 90, seed=8, staggered=False, key=("checkpoint", n))
    index = run.steps[taken_at - 1]["S"][:, lo.CMD_COUNT].view(np.uint32)
    assert (index >= 2).all() and sum(int(s["resampled"].sum()) for s in run.steps[taken_at:]) >= 3 * n
    env = LC.make_env(over, n)
    env.reset()
    for s in run.steps[:taken_at]:
        env.step(torch.from_numpy(s["a"]).to(env.device))
    same_bits(env.get_state(), run.steps[taken_at - 1]["S"], "state at the checkpoint")
    sd = env.state_dict()
    env2 = LC.make_env({**over, "seed_lo": 77, "seed_hi": 0}, n)
    env2.reset()
    env2.load_state_dict(sd)
    for k, s in enumerate(run.steps[taken_at:], taken_at):
        a = torch.from_numpy(s["a"]).to(env.device)
        o1, o2 = env.step(a)[0]["policy"], env2.step(a)[0]["policy"]
        same_bits(o2, s["obs"], f"restored env, obs step {k}")
        same_bits(o1, s["obs"], f"original env, obs step {k}")
        same_bits(env2.get_state(), s["S"], f"restored env, state step {k}")
    env.close()
    env2.close()
