"""tracker.EpisodeTracker (csrc/tracker_kernels.hip) where its loops take a second pass, against tracker.TorchEpisodeTracker with
tests/test_gpu_tracker.py's rule: every field of the state block and every written value equal, NaN matching NaN.

  * more than 65 536 envs (257 and 258 chunks of 256): tracker_commit_kernel's 256 threads take a second chunk each
  * a state block of more than 262 144 words: tracker_init_kernel's 1024 workgroups stride
  * 300 and 4096 slots: tracker_track_kernel's second workgroup, tracker_snapshot_kernel's copy loop beyond its first 256 words

The scripts have twelve steps at most (tests/tracker_cases.py), so the CPU specification runs in under a second."""
import functools

import numpy as np
import pytest
import torch

from tracker_cases import BIG_SIZES, MANY_TAGS, big_script, many_tags, same, same_writes

from isaac_rover_orbit_amd import _lib
from isaac_rover_orbit_amd import tracker as T

pytestmark = pytest.mark.gpu
FIELDS = ("cum_r", "cum_t", "ring_r", "ring_t", "head", "len", "steps", "window_steps", "sum", "max", "min", "slot_sum", "slot_count",
          "slot_max", "slot_min")


def cpu(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def dev(x):
    return cpu(x).cuda()


def assert_same_block(got: np.ndarray, want: np.ndarray, n: int, slots: int, what=""):
    g, w = T.block_views(got, n, slots), T.block_views(want, n, slots)
    for k in FIELDS:
        assert same(g[k], w[k]), (what, k)
    assert got[0] == want[0] == n and got[1] == want[1] == slots and not got[6:8].any()


@functools.lru_cache(maxsize=None)
def big_spec(n):
    """The specification on big_script(n): (writes, the block after every step)."""
    steps, interval = big_script(n)
    spec = T.TorchEpisodeTracker(n, write_interval=interval)
    writes, blocks = [], []
    for t, (rew, term, trunc) in enumerate(steps):
        spec.step(cpu(rew), cpu(term), cpu(trunc))
        blocks.append(spec.block_numpy())
        d = spec.post_interaction(t)
        if d is not None:
            writes.append((t + 1, d))
    return writes, blocks


@pytest.mark.parametrize("n", BIG_SIZES)
def test_more_than_65536_envs_take_the_commit_kernels_second_pass(n):
    steps, interval = big_script(n)
    want, blocks = big_spec(n)
    trk = T.EpisodeTracker(n, write_interval=interval)
    got = []
    for t, (rew, term, trunc) in enumerate(steps):
        trk.step(dev(rew), dev(term), dev(trunc))
        assert_same_block(trk.block_numpy(), blocks[t], n, 0, f"step {t}")
        d = trk.post_interaction(t)
        if d is not None:
            got.append((t + 1, d))
    assert len(got) == 3 and same_writes(got, want), (got, want)
    # what the script is for: the extremes of interval 1 come from the last chunk, the windows of interval 2 hold the 100 highest
    # finishers, a NaN among them, and interval 3 carries the +inf
    first, second, third = (d for _, d in got)
    assert first[T.BUILTIN_TAGS[0]] == 50.0 and first[T.BUILTIN_TAGS[1]] == -60.0 and np.isfinite(first[T.BUILTIN_TAGS[2]])
    assert np.isnan(second[T.BUILTIN_TAGS[3]]) and second[T.BUILTIN_TAGS[6]] == 7.0
    assert third[T.BUILTIN_TAGS[0]] == np.inf and third[T.BUILTIN_TAGS[5]] == np.inf
    v = T.block_views(blocks[6], n, 0)
    assert v["len"][0] == 100 and np.isnan(v["ring_r"]).sum() == 1 and not v["cum_t"][n - 1]


def test_init_strides_over_a_block_of_more_than_262144_words():
    n = 131100
    assert T.state_words(n, 0) == 262420 > 1024 * 256
    spec = T.TorchEpisodeTracker(n, write_interval=0)
    trk = T.EpisodeTracker(n, write_interval=0)
    trk.state.fill_(0x5A5A5A5A)                              # nothing of the block is right by luck
    _lib.check(trk._lib.rover_tracker_init(trk.state.data_ptr(), n, 0, trk._stream()), "rover_tracker_init")
    assert np.array_equal(trk.block_numpy(), spec.block_numpy())                 # word for word, the reserved ones too
    g = np.random.default_rng(4)
    rew = (g.standard_normal(n) * 2.0).astype(np.float32)
    term = np.zeros(n, np.float32)
    term[[0, 65535, 65536, 131071, 131072, n - 1]] = 1
    spec.step(cpu(rew), cpu(term))
    trk.step(dev(rew), dev(term))
    assert_same_block(trk.block_numpy(), spec.block_numpy(), n, 0)
    v = T.block_views(trk.block_numpy(), n, 0)
    assert v["len"][0] == 6 and v["ring_r"][5] == rew[n - 1] and (v["cum_t"] == 1).sum() == n - 6


@pytest.mark.parametrize("clear", [True, False])
@pytest.mark.parametrize("count", MANY_TAGS)
def test_many_slots_track_snapshot_and_clear(count, clear):
    """track_vector over every slot (slot i is fed i, then i + 0.5 with a NaN and a -inf among them), track on the first, the 257th
    and the last slot, a write, and a second interval that has to start clean."""
    n = 4
    tags = many_tags(count)
    trk = T.EpisodeTracker(n, tags=tags, write_interval=2, clear_window_on_write=clear)
    spec = T.TorchEpisodeTracker(n, tags=tags, write_interval=2, clear_window_on_write=clear)
    base = np.arange(count, dtype=np.float32)
    second = base + np.float32(0.5)
    second[7], second[258], second[count - 2] = np.nan, -np.inf, np.inf
    rew = np.array([0.5, -1.0, 2.0, 0.25], np.float32)
    term = np.array([0, 1, 0, 0], np.float32)
    writes = {id(trk): [], id(spec): []}
    for t in range(4):
        for k, conv in ((trk, dev), (spec, cpu)):
            k.step(conv(rew), conv(term if t == 0 else np.zeros(n, np.float32)))
            k.track_vector(tags, conv(base if t % 2 == 0 else second))
            for slot, value in ((0, -3.0 - t), (256, 1e30 * (t + 1)), (count - 1, 0.125)):
                k.track(tags[slot], value)
            d = k.post_interaction(t)
            if d is not None:
                writes[id(k)].append((t + 1, d))
        assert_same_block(trk.block_numpy(), spec.block_numpy(), n, count, f"step {t}")
    got, want = writes[id(trk)], writes[id(spec)]
    assert len(got) == 2 and same_writes(got, want)
    for i, (_, d) in enumerate(got):
        assert len(d) == (3 if clear and i else 9) + count   # every slot was fed; the windows are empty behind a clearing write
        assert np.isnan(d[tags[7]]) and d[tags[258]] == (258.0 if 258 % 3 == 0 else -np.inf) and d[tags[3]] == 3.5
        assert d[tags[count - 1]] == {0: max, 1: min}.get((count - 1) % 3, lambda *a: sum(a) / 4)(count - 1.0, 0.125, count - 0.5, 0.125)
    # the second interval started clean: its values are the first one's, but for the tags fed by track (other values) and the window
    assert all(same(got[0][1][tg], got[1][1][tg]) for tg in tags[1:256] + tags[257:count - 1])
    v = T.block_views(trk.block_numpy(), n, count)
    assert not v["slot_count"].any() and not v["slot_sum"].any() and (v["slot_max"] == -np.inf).all() and (v["slot_min"] == np.inf).all()
    assert v["len"][0] == (0 if clear else 1) and v["head"][0] == (0 if clear else 1) and v["steps"][0] == 0
    assert (T.BUILTIN_TAGS[3] in got[1][1]) == (not clear)
