"""isaac_rover_orbit_amd.tracker on the CPU: the specification of the tracker kernels (TorchEpisodeTracker) against the literal
restatement of skrl 1.1.0's tracking (SkrlTracking), the write cadence, the tags, the checkpoint and the writer.

Bounds (none of them comes from what the code gives):
  max / min of every group and every timestep statistic that is a max / min: equal.
  Total-reward mean of one step: two float64 summation orders of len <= 100 terms differ by at most 2 (len - 1) 2^-53 sum|x|, the
    two divisions add 2 * 2^-53 |mean|: within len * 2^-51 * mean|x| of numpy's value.
  Instantaneous mean of one step: the same argument at float32's unit roundoff: within n * 2^-24 * mean|r| of torch.mean in float32.
  A written mean is the mean of the per-step values over the interval: the per-step bound's maximum over the interval, plus the
    difference of two float64 summation orders of at most 60 terms (60 * 2^-52 * mean|m|).
"""
import json
import math

import numpy as np
import pytest
import torch

from tracker_cases import CASES, INFO_TAGS, USER_TAGS, run, same, same_writes, script

from isaac_rover_orbit_amd import tracker as T

INST, TOTAL, TIME = T.BUILTIN_TAGS[0:3], T.BUILTIN_TAGS[3:6], T.BUILTIN_TAGS[6:9]


def to_torch(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def run_skrl(steps, interval, clear=True):
    sk = T.SkrlTracking(interval, clear)
    writes = []
    for t, (rew, term, trunc) in enumerate(steps):
        sk.record_transition(to_torch(rew), to_torch(term), None if trunc is None else to_torch(trunc))
        d = sk.post_interaction(t)
        if d is not None:
            writes.append((t + 1, d))
    return writes, sk


@pytest.mark.parametrize("clear", [True, False])
@pytest.mark.parametrize("n", [1, 65, 257, 1000])
@pytest.mark.parametrize("case", CASES)
def test_spec_matches_skrl_at_the_writes(case, n, clear):
    steps, interval = script(case, n)
    spec = T.TorchEpisodeTracker(n, write_interval=interval, clear_window_on_write=clear)
    got = run(spec, steps, to_torch)
    want, _ = run_skrl(steps, interval, clear)
    assert [t for t, _ in got] == [t for t, _ in want] and len(got) == len(steps) // interval
    rew = np.stack([s[0] for s in steps]).astype(np.float64)
    for (t, g), (_, w) in zip(got, want):
        assert set(g) == set(w), (t, sorted(set(g) ^ set(w)))
        if case == "none":
            assert not any(k in g for k in TOTAL + TIME)
        for k in g:
            if k.endswith("(max)") or k.endswith("(min)"):
                assert same(g[k], w[k]), (t, k, g[k], w[k])
        lo = t - interval
        step_bound = max(n * 2.0 ** -24 * np.mean(np.abs(rew[i])) for i in range(lo, t))
        k = INST[2]
        if math.isnan(w[k]) or math.isinf(w[k]):
            assert same(g[k], w[k])
        else:
            print(case, n, t, k, abs(g[k] - w[k]), step_bound)
            assert abs(g[k] - w[k]) <= step_bound + 60 * 2.0 ** -52 * abs(w[k])
        if TIME[2] in g:
            assert abs(g[TIME[2]] - w[TIME[2]]) <= 60 * 2.0 ** -52 * abs(w[TIME[2]])


@pytest.mark.parametrize("n", [1, 64, 257, 1000])
@pytest.mark.parametrize("case", ["one", "all", "wrap70", "exact101", "random", "nan_inf"])
def test_per_step_means_within_the_stated_bounds(case, n):
    """A write after every step: what is written is the step's own statistics."""
    steps, _ = script(case, n)
    spec = T.TorchEpisodeTracker(n, clear_window_on_write=False)
    sk = T.SkrlTracking(1, clear_window_on_write=False)
    for t, (rew, term, trunc) in enumerate(steps):
        spec.step(to_torch(rew), to_torch(term), None if trunc is None else to_torch(trunc))
        sk.record_transition(to_torch(rew), to_torch(term), None if trunc is None else to_torch(trunc))
        g, w = spec.write(t + 1), sk.write_tracking_data(t + 1)
        assert set(g) == set(w)
        for k in g:
            if not k.endswith("(mean)"):
                assert same(g[k], w[k]), (t, k)
        tm = float(torch.mean(to_torch(rew)))
        assert same(w[INST[2]], tm)
        if math.isfinite(tm):
            assert abs(g[INST[2]] - tm) <= n * 2.0 ** -24 * float(np.mean(np.abs(rew.astype(np.float64))))
        else:
            assert same(g[INST[2]], tm)
        if TOTAL[2] in g:
            win = np.array(sk._track_rewards)
            assert len(win) == int(spec.v["len"][0]) <= 100
            if np.all(np.isfinite(win)):
                assert abs(g[TOTAL[2]] - np.mean(win)) <= len(win) * 2.0 ** -51 * np.mean(np.abs(win))
            else:
                assert same(g[TOTAL[2]], np.mean(win))
            assert g[TIME[2]] == np.mean(np.array(sk._track_timesteps))


def test_window_holds_the_last_100_in_env_order():
    steps, _ = script("all", 1000)
    spec = T.TorchEpisodeTracker(1000, write_interval=1000)
    for rew, term, trunc in steps[:6]:
        spec.step(to_torch(rew), to_torch(term), to_torch(trunc))
    v = spec.v
    assert v["len"][0] == 100 and v["head"][0] == 1000 % 100
    want = np.sum(np.stack([s[0] for s in steps[:6]]).astype(np.float32)[:, 900:], axis=0, dtype=np.float32)
    order = (v["head"][0] - 100 + np.arange(100)) % 100
    cum = np.zeros(1000, np.float32)
    for s in steps[:6]:
        cum += s[0]
    assert np.array_equal(v["ring_r"][order], cum[900:]) and np.allclose(want, cum[900:], atol=1e-4)
    assert np.array_equal(v["ring_t"][order], np.full(100, 6)) and not v["cum_t"].any() and not v["cum_r"].any()


@pytest.mark.parametrize("clear", [True, False])
def test_clear_window_on_write_is_a_switch(clear):
    steps, interval = script("write_between", 65)
    spec = T.TorchEpisodeTracker(65, write_interval=interval, clear_window_on_write=clear)
    writes = dict(run(spec, steps, to_torch))
    assert sorted(writes) == [10, 20, 30]
    assert TOTAL[0] in writes[10] and TOTAL[0] in writes[20]
    # env 0 finished at steps 5 (length 6) and 15 (length 10); nothing finishes after step 15
    assert writes[10][TIME[0]] == 6.0 and writes[20][TIME[0]] == 10.0
    assert writes[20][TIME[1]] == (10.0 if clear else 6.0)
    assert (TOTAL[0] in writes[30]) == (not clear)
    assert spec.v["len"][0] == (0 if clear else 2)
    assert spec.v["cum_t"][0] == 32 - 16 and spec.v["cum_t"][1] == 32      # a write keeps cum_r / cum_t


def test_write_cadence():
    spec = T.TorchEpisodeTracker(4, write_interval=1)
    z = torch.zeros(4)
    spec.step(z, z)
    assert spec.post_interaction(0) is None                 # timestep + 1 == 1 never writes
    spec.step(z, z)
    assert spec.post_interaction(1) is not None
    seen = []
    spec = T.TorchEpisodeTracker(4, write_interval=7, callback=lambda d, s: seen.append((s, d)))
    out = []
    for t in range(30):
        spec.step(z + t, z)
        d = spec.post_interaction(t)
        if d is not None:
            out.append((t + 1, d))
    assert [s for s, _ in out] == [7, 14, 21, 28] and seen == out
    assert out[1][1][INST[0]] == 13.0 and out[1][1][INST[1]] == 7.0 and out[1][1][INST[2]] == 10.0
    off = T.TorchEpisodeTracker(4, write_interval=0)
    off.step(z, z)
    assert all(off.post_interaction(t) is None for t in range(5))


def test_user_tags_follow_the_suffix_rule_and_empty_tags_are_absent():
    spec = T.TorchEpisodeTracker(3, tags=USER_TAGS + INFO_TAGS, write_interval=4)
    sk = T.SkrlTracking(4)
    z = torch.zeros(3)
    vals = [1.5, -2.0, 7.25]
    for t in range(8):
        spec.step(z, z)
        sk.record_transition(z, z, z)
        if t < 3:
            for tag in USER_TAGS:
                spec.track(tag, vals[t])
                sk.track_data(tag, vals[t])
        if t >= 4:
            vec = torch.arange(16, dtype=torch.float32) * (t - 3)
            spec.track_vector(INFO_TAGS, vec)
            for tag, x in zip(INFO_TAGS, vec.tolist()):
                sk.track_data(tag, x)
        g, w = spec.post_interaction(t), sk.post_interaction(t)
        if t == 3:
            assert g[USER_TAGS[0]] == 7.25 and g[USER_TAGS[1]] == -2.0 and g[USER_TAGS[2]] == pytest.approx(2.25, abs=1e-15)
            assert not any(k in g for k in INFO_TAGS) and g == w
        if t == 7:
            assert not any(k in g for k in USER_TAGS)
            assert g[INFO_TAGS[2]] == 2.0 * (1 + 2 + 3 + 4) / 4 and set(g) == set(w)
            assert all(g[k] == pytest.approx(w[k], rel=1e-15) for k in g)
    assert T.reduction_of("x (min)") == "min" and T.reduction_of("x (max)") == "max" and T.reduction_of("x (mean) y") == "mean"


def test_undeclared_tag_raises():
    spec = T.TorchEpisodeTracker(3, tags=USER_TAGS)
    with pytest.raises(KeyError):
        spec.track("Loss / Policy loss", 1.0)
    with pytest.raises(KeyError):
        spec.track_vector(("nope",), torch.zeros(16))
    with pytest.raises(ValueError):
        spec.track_vector((USER_TAGS[1], USER_TAGS[0]), torch.zeros(16))       # not in declared order
    with pytest.raises(ValueError):
        T.TorchEpisodeTracker(3, tags=("a", "a"))
    with pytest.raises(ValueError):
        T.TorchEpisodeTracker(3, tags=(T.BUILTIN_TAGS[0],))


@pytest.mark.parametrize("cut", [13, 22])
def test_state_dict_resumes_exactly(cut):
    """cut 13: in the middle of episodes and of a window (before the write at 16); cut 22: behind a write, windows refilling."""
    steps, interval = script("random", 257)
    a = T.TorchEpisodeTracker(257, tags=USER_TAGS, write_interval=interval)
    whole = run(a, steps, to_torch, user_calls=3)
    b = T.TorchEpisodeTracker(257, tags=USER_TAGS, write_interval=interval)
    first = run(b, steps[:cut], to_torch, user_calls=3)
    sd = json.loads(json.dumps({k: (v.tolist() if isinstance(v, torch.Tensor) else v) for k, v in b.state_dict().items()}))
    c = T.TorchEpisodeTracker(257, tags=USER_TAGS, write_interval=interval)
    c.load_state_dict(sd)
    assert np.array_equal(c.block, b.block)
    # the rest of the script with its own timesteps; the user values of run() restart, so compare the built-in tags
    rest = []
    for t in range(cut, len(steps)):
        rew, term, trunc = steps[t]
        c.step(to_torch(rew), to_torch(term), to_torch(trunc))
        d = c.post_interaction(t)
        if d is not None:
            rest.append((t + 1, d))
    strip = lambda ws: [(t, {k: v for k, v in d.items() if k in T.BUILTIN_TAGS}) for t, d in ws]  # noqa: E731
    assert same_writes(strip(first + rest), strip(whole))
    va, vc = a.v, c.v
    for k in ("cum_r", "cum_t", "ring_r", "ring_t", "head", "len"):
        assert same(va[k], vc[k]), k
    with pytest.raises(ValueError):
        T.TorchEpisodeTracker(256, tags=USER_TAGS).load_state_dict(sd)


def test_jsonl_writer_round_trip(tmp_path):
    path = tmp_path / "curves.jsonl"
    w = T.JsonlWriter(str(path))
    steps, interval = script("one", 65)
    spec = T.TorchEpisodeTracker(65, write_interval=interval, writer=w)
    writes = run(spec, steps, to_torch)
    w.close()
    rows = [json.loads(line) for line in open(path)]
    assert rows and all(set(r) == {"tag", "value", "step"} for r in rows)
    want = [(t, k, v) for t, d in writes for k, v in d.items()]
    assert [(r["step"], r["tag"], r["value"]) for r in rows] == want


def test_episode_info_tags_and_mirrors():
    from isaac_rover_orbit_amd import _lib, build
    from isaac_rover_orbit_amd.envs.rover_env import LOG_KEYS
    build.build_extension()
    tags = T.episode_info_tags(LOG_KEYS)
    assert len(tags) == 13 <= _lib.LOG_WORDS and tags[0] == "EpisodeInfo / " + LOG_KEYS[0]
    lib = _lib.load()
    for n, s in ((1, 0), (257, 3), (4096, 33)):
        assert lib.rover_tracker_state_bytes(n, s) == 4 * T.state_words(n, s)
        assert lib.rover_tracker_snapshot_words(s) == T.ACC_WORDS + 6 * s
        assert lib.rover_tracker_workspace_bytes(n) == (20 * -(-n // 256) + 7) // 8 * 8
    assert lib.rover_tracker_state_bytes(0, 0) == 0 and lib.rover_tracker_state_bytes(4, T.MAX_SLOTS + 1) == 0
    assert lib.rover_tracker_workspace_bytes(0) == 0
    assert {"rover_tracker_step", "rover_tracker_track", "rover_tracker_snapshot", "rover_tracker_init"} <= set(_lib.EXPORTS)
    # bad arguments are codes on any host: nothing is launched
    assert lib.rover_tracker_step(None, 4, 0, None, None, None, 4, None, 0, None) == 1
    assert lib.rover_tracker_track(None, 4, 0, 0, None, 1, None) == 1
