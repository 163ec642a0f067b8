"""tracker.EpisodeTracker (csrc/tracker_kernels.hip) against tracker.TorchEpisodeTracker, bit for bit: every written value, and
cum_r, cum_t, the rings, head and len behind the script.  "Bit for bit" is value equality of every float with NaN matching NaN: the
bit pattern of a NaN that an addition produces is the processor's choice (x86 gives the negative quiet NaN, gfx950 the positive).

The sizes cover one lane, the wave edge (63 / 64 / 65), the workgroup edge (256 / 257) and several workgroups (1000)."""
import functools
import types

import numpy as np
import pytest
import torch

from tracker_cases import CASES, INFO_TAGS, SIZES, USER_TAGS, run, same, same_writes, script

from isaac_rover_orbit_amd import tracker as T

pytestmark = pytest.mark.gpu
FIELDS = ("cum_r", "cum_t", "ring_r", "ring_t", "head", "len", "steps", "window_steps", "sum", "max", "min", "slot_sum", "slot_count",
          "slot_max", "slot_min")
TOTAL, TIME = T.BUILTIN_TAGS[3:6], T.BUILTIN_TAGS[6:9]


def cpu(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def dev(x):
    return cpu(x).cuda()


@functools.lru_cache(maxsize=None)
def spec_run(case, n, tags=(), user_calls=0, info=False, clear=True):
    steps, interval = script(case, n)
    spec = T.TorchEpisodeTracker(n, tags=tags, write_interval=interval, clear_window_on_write=clear)
    return run(spec, steps, cpu, user_calls, info), spec.block_numpy()


def assert_same_block(got: np.ndarray, want: np.ndarray, n: int, slots: int):
    g, w = T.block_views(got, n, slots), T.block_views(want, n, slots)
    for k in FIELDS:
        assert same(g[k], w[k]), k
    assert got[0] == want[0] == n and got[1] == want[1] == slots


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", CASES)
def test_device_matches_the_specification(case, n):
    steps, interval = script(case, n)
    want, block = spec_run(case, n)
    trk = T.EpisodeTracker(n, write_interval=interval)
    got = run(trk, steps, dev)
    assert len(got) == len(steps) // interval
    assert same_writes(got, want), (got, want)
    assert_same_block(trk.block_numpy(), block, n, 0)
    if case == "none":
        assert all(not any(k in d for k in TOTAL + TIME) for _, d in got)


def test_all_thousand_finish_in_one_step():
    """Only the 100 highest env ids remain, in env order."""
    steps, _ = script("all", 1000)
    trk = T.EpisodeTracker(1000, write_interval=0)
    cum = np.zeros(1000, np.float32)
    for rew, term, trunc in steps[:6]:
        trk.step(dev(rew), dev(term), dev(trunc))
        cum += rew
    v = T.block_views(trk.block_numpy(), 1000, 0)
    assert v["len"][0] == 100 and v["head"][0] == 0
    assert np.array_equal(v["ring_r"], cum[900:]) and np.array_equal(v["ring_t"], np.full(100, 6))
    assert not v["cum_r"].any() and not v["cum_t"].any()


@pytest.mark.parametrize("n", [65, 1000])
@pytest.mark.parametrize("kind", [torch.bool, torch.uint8])
def test_byte_flags_as_the_envs_return_them(kind, n):
    steps, interval = script("random", n)
    want, block = spec_run("random", n)
    trk = T.EpisodeTracker(n, write_interval=interval)
    got = []
    for t, (rew, term, trunc) in enumerate(steps):
        trk.step(dev(rew), dev(term != 0).to(kind), dev(trunc != 0).to(kind))
        d = trk.post_interaction(t)
        if d is not None:
            got.append((t + 1, d))
    assert same_writes(got, want)
    assert_same_block(trk.block_numpy(), block, n, 0)


@pytest.mark.parametrize("clear", [True, False])
@pytest.mark.parametrize("user_calls", [0, 3])
def test_track_and_track_vector(user_calls, clear):
    """Slots with a (max), a (min) and a mean tag, never fed and fed three times per interval, beside the 16-float log vector."""
    n, tags = 257, USER_TAGS + INFO_TAGS
    steps, interval = script("random", n)
    want, block = spec_run("random", n, tags, user_calls, True, clear)
    trk = T.EpisodeTracker(n, tags=tags, write_interval=interval, clear_window_on_write=clear)
    got = run(trk, steps, dev, user_calls, True)
    assert same_writes(got, want)
    assert_same_block(trk.block_numpy(), block, n, len(tags))
    assert all((USER_TAGS[0] in d) == (user_calls > 0) and INFO_TAGS[15] in d for _, d in got)
    with pytest.raises(KeyError):
        trk.track("Loss / Policy loss", 1.0)


def test_track_reads_device_values_where_they_lie():
    trk = T.EpisodeTracker(4, tags=USER_TAGS, write_interval=2)
    spec = T.TorchEpisodeTracker(4, tags=USER_TAGS, write_interval=2)
    vals = torch.tensor([3.5, float("nan"), -1.25, float("inf")], device="cuda")
    z = torch.zeros(4, device="cuda")
    for t in range(2):
        for k in (trk, spec):
            k.step(z, z)
            k.track(USER_TAGS[0], vals[2 * t:2 * t + 1])
            k.track(USER_TAGS[2], vals[2 * t + 1:2 * t + 2])
    g, w = trk.post_interaction(1), spec.post_interaction(1)
    assert list(g) == list(w) and all(same(g[k], w[k]) for k in g)
    assert g[USER_TAGS[0]] == 3.5 and np.isnan(g[USER_TAGS[2]]) and USER_TAGS[1] not in g


def test_ppo_scalars_from_device_statistics():
    stats = torch.full((2, 3, 4), float("nan"), device="cuda")
    stats[0] = torch.tensor([[0.01, 1.0, 2.0, 0.0], [0.02, 3.0, 4.0, 0.0], [0.03, 5.0, 6.0, 0.0]], device="cuda")
    stats[1, 0] = torch.tensor([0.04, 7.0, 8.0, 0.0], device="cuda")            # the early stop skipped the last two minibatches
    state = torch.zeros(4, dtype=torch.float64, device="cuda")
    state[0] = 2.5e-4
    trainer = types.SimpleNamespace(last_stats=stats, log_std=torch.log(torch.tensor([0.5, 0.25], device="cuda")), state=state)
    trk = T.EpisodeTracker(4, tags=T.PPO_TAGS, write_interval=1)
    z = torch.zeros(4, device="cuda")
    trk.step(z, z)
    T.track_ppo_update(trk, trainer)
    d = trk.post_interaction(1)
    assert d["Loss / Policy loss"] == pytest.approx(16.0 / 6.0, rel=1e-6) and d["Loss / Value loss"] == pytest.approx(20.0 / 6.0, rel=1e-6)
    assert d["Policy / Standard deviation"] == pytest.approx(0.375, rel=1e-6) and d["Learning / Learning rate"] == float(np.float32(2.5e-4))


def test_nothing_synchronises_between_writes():
    """step, track_vector, track on a device value, track_ppo_update and the post_interaction of a step that does not write run
    under torch's synchronisation check; the write itself is the one read-back."""
    n = 257
    steps, _ = script("random", n)
    trk = T.EpisodeTracker(n, tags=INFO_TAGS + T.PPO_TAGS, write_interval=8)
    data = [tuple(dev(x) for x in s) for s in steps[:8]]
    vec, one = torch.arange(16, dtype=torch.float32, device="cuda"), torch.ones(1, device="cuda")
    state = torch.zeros(4, dtype=torch.float64, device="cuda")
    trainer = types.SimpleNamespace(last_stats=torch.ones(2, 3, 4, device="cuda"), log_std=torch.zeros(2, device="cuda"), state=state)
    T.track_ppo_update(trk, trainer)                         # every torch kernel of the window has run once
    trk.write(0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for t in range(7):
            trk.step(*data[t])
            trk.track_vector(INFO_TAGS, vec)
            trk.track(INFO_TAGS[0], one)
            assert trk.post_interaction(t) is None
        T.track_ppo_update(trk, trainer)
        trk.step(*data[7])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    d = trk.post_interaction(7)
    assert d is not None and d[INFO_TAGS[3]] == 3.0 and d[T.PPO_TAGS[0]] == 1.0
    assert d[T.BUILTIN_TAGS[0]] == max(float(s[0].max()) for s in steps[:8])


def test_stale_workspace_does_not_matter():
    n = 1000
    steps, interval = script("random", n)
    want, block = spec_run("random", n)
    trk = T.EpisodeTracker(n, write_interval=interval)
    got = []
    for t, (rew, term, trunc) in enumerate(steps):
        trk.ws.fill_(0xFF)                                   # NaN bytes, counts of -1
        trk.step(dev(rew), dev(term), dev(trunc))
        d = trk.post_interaction(t)
        if d is not None:
            got.append((t + 1, d))
    assert same_writes(got, want)
    assert_same_block(trk.block_numpy(), block, n, 0)


def test_two_trackers_on_two_streams():
    na, nb = 257, 1000
    (sa, ia), (sb, ib) = script("random", na), script("wrap70", nb)
    a, b = T.EpisodeTracker(na, write_interval=ia), T.EpisodeTracker(nb, write_interval=ib)
    da = [tuple(dev(x) for x in s) for s in sa]
    db = [tuple(dev(x) for x in s) for s in sb]
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ga, gb = [], []
    for t in range(max(len(da), len(db))):
        for trk, data, stream, out in ((a, da, s1, ga), (b, db, s2, gb)):
            if t < len(data):
                with torch.cuda.stream(stream):
                    trk.step(*data[t])
                    d = trk.post_interaction(t)
                if d is not None:
                    out.append((t + 1, d))
    torch.cuda.synchronize()
    (wa, ba), (wb, bb) = spec_run("random", na), spec_run("wrap70", nb)
    assert same_writes(ga, wa) and same_writes(gb, wb)
    assert_same_block(a.block_numpy(), ba, na, 0)
    assert_same_block(b.block_numpy(), bb, nb, 0)


def test_state_dict_moves_between_the_device_and_the_specification():
    n = 257
    steps, interval = script("random", n)
    spec = T.TorchEpisodeTracker(n, tags=USER_TAGS, write_interval=interval)
    for rew, term, trunc in steps[:13]:                      # in the middle of episodes and of a window
        spec.step(cpu(rew), cpu(term), cpu(trunc))
    trk = T.EpisodeTracker(n, tags=USER_TAGS, write_interval=interval)
    trk.load_state_dict(spec.state_dict())
    for rew, term, trunc in steps[13:29]:
        for k, conv in ((spec, cpu), (trk, dev)):
            k.step(conv(rew), conv(term), conv(trunc))
    back = T.TorchEpisodeTracker(n, tags=USER_TAGS, write_interval=interval)
    back.load_state_dict(trk.state_dict())
    assert_same_block(back.block, spec.block, n, 3)
    g, w = trk.write(29), spec.write(29)
    assert list(g) == list(w) and all(same(g[k], w[k]) for k in g)
    with pytest.raises(ValueError):
        T.EpisodeTracker(n + 1, tags=USER_TAGS).load_state_dict(spec.state_dict())


def test_bad_arguments_are_codes_and_leave_the_state_untouched():
    n = 300
    trk = T.EpisodeTracker(n, tags=USER_TAGS)
    lib = trk._lib
    steps, _ = script("random", 1000)
    trk.step(dev(steps[0][0][:n]), dev(steps[0][1][:n]), dev(steps[0][2][:n]))
    before = trk.block_numpy()
    rew, term = dev(steps[1][0][:n]), dev(steps[1][1][:n])
    vals = torch.ones(4, device="cuda")
    p = lambda t: t.data_ptr()  # noqa: E731
    small = int(lib.rover_tracker_workspace_bytes(n)) - 8
    INVALID = 1
    assert lib.rover_tracker_step(p(trk.state), 0, 3, p(rew), p(term), None, 4, p(trk.ws), trk.ws.numel(), None) == INVALID
    assert lib.rover_tracker_step(p(trk.state), n, 3, p(rew), p(term), None, 4, p(trk.ws), small, None) == INVALID
    assert b"workspace" in lib.rover_last_error()
    assert lib.rover_tracker_step(p(trk.state), n, 3, p(rew), p(term), None, 2, p(trk.ws), trk.ws.numel(), None) == INVALID
    assert lib.rover_tracker_step(p(trk.state), n, 3, None, p(term), None, 4, p(trk.ws), trk.ws.numel(), None) == INVALID
    assert lib.rover_tracker_track(p(trk.state), n, 3, 3, p(vals), 1, None) == INVALID          # slot 3 of 3
    assert lib.rover_tracker_track(p(trk.state), n, 3, 2, p(vals), 2, None) == INVALID          # runs past the last slot
    assert lib.rover_tracker_track(p(trk.state), n, 3, -1, p(vals), 1, None) == INVALID
    assert lib.rover_tracker_track(p(trk.state), n, 3, 0, p(vals), 0, None) == INVALID
    assert lib.rover_tracker_snapshot(p(trk.state), n, 3, None, 1, None) == INVALID
    assert lib.rover_tracker_init(p(trk.state), n, T.MAX_SLOTS + 1, None) == INVALID
    torch.cuda.synchronize()
    assert np.array_equal(trk.block_numpy(), before)
    with pytest.raises(ValueError):
        trk.step(rew[:-1], term[:-1])
    with pytest.raises(ValueError):
        trk.step(rew.double(), term)
    with pytest.raises(ValueError):
        trk.step(rew, term, term.bool())
    assert np.array_equal(trk.block_numpy(), before)
