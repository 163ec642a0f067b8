"""The fused episode recorder (isaac_rover_orbit_amd.trace_collect.TraceCollector, include/rover_trace.h) against the specification
(trace.EpisodeRecorder) on the GPU: identical files, bit for bit, for identical per-step tensors.

  * env counts around a wave, a workgroup and the commit kernel's 256-env chunk
  * row widths of 3860, 8, 4, 1, 40 and 3 bytes, and one 57 600-byte extra, contiguous and as the camera's permuted view
  * an observation source 4 bytes off a 16-byte boundary
  * ring wrap with pieces of 7 rows, 1 row and more rows than are ever emitted
  * all envs done in one step, none done for whole intervals, only the last env done
  * NaN payloads, -0.0 and infinities survive
  * two collectors in one process; overflow raises at the drain with every canary intact
  * the per-step path is two launches in one C call and never synchronises
  * 16 envs of RoverEnv for 40 steps with time-outs: fused and host recorders write the same files
"""
import numpy as np
import pytest
import torch

from trace_cases import EXTRAS, assert_same_files, drive, step_tensors

from isaac_rover_orbit_amd import trace_collect as TC
from isaac_rover_orbit_amd.trace import EpisodeRecorder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KW = dict(max_episode_rows=6, drain_interval=3, piece_rows=7)


def _make(n, obs_dim=965, extras=EXTRAS, max_rows=40, **kw):
    args = dict(KW, **kw)
    return lambda base: TC.TraceCollector(base, n, obs_dim, 2, extras, max_rows=max_rows, device=DEV, **args)


def _run(tmp_path, n, steps=40, p_done=0.15, obs_dim=965, extras=EXTRAS, max_rows=None, make_kw=None, **kw):
    max_rows = (40 if n <= 5 else 1000) if max_rows is None else max_rows
    ref, col, fr, fg = drive(_make(n, obs_dim, extras, max_rows, **(make_kw or {})), str(tmp_path), n, steps, p_done, 6, obs_dim=obs_dim,
                             extras=extras, max_rows=max_rows, device=DEV, **kw)
    return col, assert_same_files(fr, fg)


@pytest.mark.parametrize("n", [1, 5, 67, 130, TC.COMMIT_CHUNK - 1, TC.COMMIT_CHUNK, TC.COMMIT_CHUNK + 1])
def test_env_counts_and_row_widths(tmp_path, n):
    """965 floats, 2 floats, 4 B, 1 B, a 40-byte and a 3-byte extra; rings of 9 rows wrap, pieces of 7 rows cut episodes."""
    col, steps = _run(tmp_path, n)
    assert sum(steps) == 40 * n and (len(steps) > 1 or n == 1)


@pytest.mark.parametrize("permuted", [False, True])
def test_wide_extra(tmp_path, permuted):
    """One 57 600-byte extra at n = 3: 15 spans per row.  ``permuted``: the layout of RoverEnvCamera's extras["depth"]."""
    ex = {"depth": {"shape": (160, 90), "dtype": np.float32}}
    put = None
    if permuted:
        def put(name, x):
            return x.permute(0, 2, 1).contiguous().to(DEV).permute(0, 2, 1) if name == "depth" else x.to(DEV)
    col, steps = _run(tmp_path, 3, steps=14, obs_dim=7, extras=ex, to_device=put)
    assert sum(steps) == 42


def test_misaligned_observation_source(tmp_path):
    n = 5
    seen = []

    def put(name, x):
        if name != "obs":
            return x.to(DEV)
        buf = torch.empty(n * 965 + 4, device=DEV)
        v = buf[1:1 + n * 965].view(n, 965)
        v.copy_(x)
        seen.append(v.data_ptr() % 16)
        return v
    col, steps = _run(tmp_path, n, to_device=put)
    assert set(seen) == {4}


@pytest.mark.parametrize("piece", [1, 256])
def test_piece_edges(tmp_path, piece):
    """Pieces of one row, and one piece larger than everything a drain emits (at most 5 x 9 rows)."""
    _run(tmp_path, 5, make_kw=dict(piece_rows=piece))


@pytest.mark.parametrize("pattern", ["all_in_one_step", "none_for_an_interval", "last_env_only"])
def test_done_patterns(tmp_path, pattern):
    n = 67
    fn = {"all_in_one_step": lambda t, n_: torch.full((n_,), t == 4),
          "none_for_an_interval": lambda t, n_: torch.full((n_,), t % 6 == 5),
          "last_env_only": lambda t, n_: torch.arange(n_) == n_ - 1}[pattern]
    col, steps = _run(tmp_path, n, steps=20, done_fn=fn)
    assert sum(steps) == 20 * n


def test_special_values_survive(tmp_path):
    col, steps = _run(tmp_path, 5, special=True)
    from isaac_rover_orbit_amd.trace import load_trace
    d = load_trace(col.writer.files[0])
    obs_bits, rew_bits = d["observations"].view(np.uint32), d["rewards"].view(np.uint32)
    for bits in (0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x7F800000, 0xFF800000):
        assert (obs_bits == bits).any(), hex(bits)
    assert np.isin(rew_bits, [0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x7F800000, 0xFF800000]).all()


def test_two_collectors_leave_each_other_alone(tmp_path):
    """A second collector of another shape, interleaved step by step with the first (same stream, same process), then one more
    created after both closed: every file still equals the specification's."""
    n1, n2 = 5, 67
    hook_state = {}

    def hook(col, t):
        if "other" not in hook_state:
            hook_state["g"] = torch.Generator().manual_seed(99)
            (tmp_path / "r2").mkdir()
            (tmp_path / "d2").mkdir()
            hook_state["ref"] = EpisodeRecorder(str(tmp_path / "r2" / "run"), n2, 11, 2, None, max_rows=300)
            hook_state["other"] = TC.TraceCollector(str(tmp_path / "d2" / "run"), n2, 11, 2, None, max_rows=300, device=DEV,
                                                    max_episode_rows=40, drain_interval=5, piece_rows=64)
        obs, act, rew, _ = step_tensors(hook_state["g"], n2, 11, 2, None)
        done = torch.rand(n2, generator=hook_state["g"]) < 0.2
        hook_state["ref"].append_to_buffer(obs, act, rew, done)
        hook_state["other"].append(obs.to(DEV), act.to(DEV), rew.to(DEV), done.to(DEV))
    col, steps = _run(tmp_path / "a", n1, hook=hook)
    assert_same_files(hook_state["ref"].close(), hook_state["other"].close())
    _run(tmp_path / "b", n1, seed=3)


def test_overflow_is_raised_at_drain_and_bounds_are_kept(tmp_path):
    """Env 1 is never done: its 7th row is refused (nothing is overwritten), the status sticks, the next drain raises, and the
    canary bytes behind the state block, every ring and every output block are intact.  What the earlier drains wrote stays."""
    n = 5
    done_fn = lambda t, n_: torch.tensor([t % 2 == 1 and e != 1 for e in range(n_)])   # noqa: E731
    ref, col, _, _ = drive(_make(n, max_rows=500, guard_bytes=64), str(tmp_path), n, 6, 0.0, 6, obs_dim=965, max_rows=500, device=DEV,
                           done_fn=done_fn, force=False, close=False)
    g = torch.Generator().manual_seed(5)
    obs, act, rew, info = step_tensors(g, n, 965, 2, EXTRAS)
    for _ in range(2):                                                                 # rows 7 and 8 of env 1
        col.append(obs.to(DEV), act.to(DEV), rew.to(DEV), torch.zeros(n, dtype=torch.bool, device=DEV), {k: v.to(DEV) for k, v in info.items()})
    with pytest.raises(TC.TraceOverflowError, match="max_episode_rows"):
        col.drain()
    assert col.guards_intact()
    got = col.close()
    ref._close_file()
    assert assert_same_files(ref.files, got) == [24]
    col2, _ = _run(tmp_path / "ok", 67, make_kw=dict(guard_bytes=64))                  # and in a run that does not overflow
    assert col2.guards_intact()


def test_per_step_path_is_two_launches_and_no_sync(tmp_path):
    """The existing collectors' tests make no launch-count or no-sync check, so: the wrapper's own call log shows one
    rover_trace_append (two launches: include/rover_trace.h) per step and nothing else, and torch's sync debug mode raises on any
    synchronising call made between the appends."""
    n, k = 130, 7
    col = TC.TraceCollector(str(tmp_path / "run"), n, 965, 2, EXTRAS, max_rows=10_000, device=DEV, max_episode_rows=20, drain_interval=8)
    g = torch.Generator().manual_seed(1)
    steps = []
    for t in range(k):
        obs, act, rew, info = step_tensors(g, n, 965, 2, EXTRAS)
        steps.append((obs.to(DEV), act.to(DEV), rew.to(DEV), (torch.rand(n, generator=g) < 0.3).to(DEV), {k_: v.to(DEV) for k_, v in info.items()}))
    torch.cuda.synchronize()
    assert col.calls == [("rover_trace_init", 0)]
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            steps[0][2].sum().item()                                                   # the detector works
        for s in steps:
            col.append(*s)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert col.calls[1:] == [("rover_trace_append", 2)] * k and max(c[1] for c in col.calls) <= 2
    col.drain()
    names = [c[0] for c in col.calls[1 + k:]]
    assert names[-1] == "rover_trace_drained" and set(names[:-1]) == {"rover_trace_gather"}
    col.close()


def test_end_to_end_rover_env(tmp_path):
    """16 envs, 40 steps, zero agent, 1 s episodes (time-outs every 5 steps): the loop of examples/08_collect_traces.py."""
    from isaac_rover_orbit_amd import terrain as T
    from isaac_rover_orbit_amd.cfg import RoverEnvCfg
    from isaac_rover_orbit_amd.envs import RoverEnv
    n = 16
    ter = T.make_procedural_terrain((512, 512), seed=21, n_rocks=40)
    ter.make_spawns(2 * 2048, border_offset=2.0)
    cfg = RoverEnvCfg()
    cfg.scene.num_envs, cfg.sim.device, cfg.terrain.kind, cfg.episode_length_s = n, DEV, "custom", 1.0
    env = RoverEnv(cfg, terrain=ter)
    host = EpisodeRecorder(str(tmp_path / "host"), n, 965, 2, max_rows=150)
    fused = TC.TraceCollector(str(tmp_path / "fused"), n, 965, 2, max_rows=150, env=env, drain_interval=8, device=DEV)
    assert fused.max_ep == env.max_episode_length == 5
    obs, _ = env.reset()
    actions = torch.zeros(n, 2, device=DEV)
    ndone = 0
    for _ in range(40):
        nxt, rew, terminated, truncated, info = env.step(actions)
        done = terminated | truncated
        host.append_to_buffer(obs["policy"], actions, rew, done)
        fused.append(obs["policy"], actions, rew, done)
        ndone += int(done.sum())
        obs = nxt
    fh, ff = host.close(), fused.close()
    env.close()
    assert ndone >= n * 7
    import os
    assert [os.path.basename(f).replace("fused", "host") for f in ff] == [os.path.basename(f) for f in fh]
    from isaac_rover_orbit_amd.trace import load_trace
    total = 0
    for a, b in zip(fh, ff):
        x, y = load_trace(a), load_trace(b)
        assert sorted(x) == sorted(y) and x["number_of_steps"] == y["number_of_steps"]
        total += x["number_of_steps"]
        for key in x:
            if key != "number_of_steps":
                assert x[key].dtype == y[key].dtype and x[key].shape == y[key].shape
                assert np.array_equal(np.ascontiguousarray(x[key]).reshape(-1).view(np.uint8), np.ascontiguousarray(y[key]).reshape(-1).view(np.uint8)), key
    assert total == 40 * n and len(fh) >= 4
