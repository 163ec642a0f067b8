"""Scripted step sequences shared by tests/test_tracker.py and tests/test_gpu_tracker.py (not a test module).

A script is a list of steps ``(rew, terminated, truncated)``: float32 numpy arrays of ``n`` values, ``truncated`` possibly None.
Rewards come from a seeded generator; who finishes when is written out per case."""
import functools

import numpy as np

SIZES = (1, 63, 64, 65, 256, 257, 1000)
USER_TAGS = ("Stat / a (max)", "Stat / b (min)", "Stat / c")
INFO_TAGS = tuple(f"EpisodeInfo / word {i}" for i in range(16))


def _blank(n, steps, seed):
    g = np.random.default_rng(seed)
    rew = (g.standard_normal((steps, n)) * 2.0 - 0.25).astype(np.float32)
    return rew, np.zeros((steps, n), np.float32), np.zeros((steps, n), np.float32)


def _first(n, k):
    return np.arange(min(n, k))


def _last(n, k):
    return np.arange(max(0, n - k), n)


@functools.lru_cache(maxsize=None)
def script(case: str, n: int):
    """Returns (steps, write_interval).  30-60 steps each."""
    interval = 16
    drop_trunc = False
    if case == "none":
        rew, term, trunc = _blank(n, 40, 1)
    elif case == "one":
        rew, term, trunc = _blank(n, 40, 2)
        term[7, n // 2] = 1
        trunc[30, n // 2] = 1
    elif case == "all":                              # with n = 1000 only the 100 highest env ids remain, in order
        rew, term, trunc = _blank(n, 36, 3)
        trunc[5, :] = 1
    elif case == "wrap70":                           # 70, then 70 more: the ring wraps across steps
        rew, term, trunc = _blank(n, 40, 4)
        term[10, _first(n, 70)] = 1
        term[20, _last(n, 70)] = 1
    elif case in ("exact100", "exact101"):
        rew, term, trunc = _blank(n, 34, 5)
        k = 100 if case == "exact100" else 101
        term[12, _first(n, k)] = 1
        trunc[25, _last(n, 3)] = 1
    elif case == "both":                             # terminated and truncated at once: finishes once
        rew, term, trunc = _blank(n, 36, 6)
        e = min(3, n - 1)
        term[9, e] = 1
        trunc[9, e] = 1
        term[9, n - 1] = 1
    elif case == "trunc_none":
        rew, term, trunc = _blank(n, 36, 7)
        term[4, _first(n, 5)] = 1
        term[22, _last(n, 2)] = 1
        drop_trunc = True
    elif case == "write_between":                    # a write (step 10) between two finishes of env 0 (steps 5 and 15)
        rew, term, trunc = _blank(n, 32, 8)
        interval = 10
        term[5, 0] = 1
        trunc[15, 0] = 1
    elif case == "nan_inf":                          # a NaN and a +inf reward in one env, followed until it finishes and on
        rew, term, trunc = _blank(n, 50, 9)
        e = n // 3
        rew[3, e] = np.nan
        rew[4, e] = np.inf
        term[20, e] = 1
        term[6, n - 1] = 1
    elif case == "random":
        rew, term, trunc = _blank(n, 60, 10)
        g = np.random.default_rng(11)
        term[:] = g.random((60, n)) < 0.03
        trunc[:] = g.random((60, n)) < 0.02
    else:
        raise KeyError(case)
    steps = [(rew[t], term[t], None if drop_trunc else trunc[t]) for t in range(len(rew))]
    return steps, interval


CASES = ("none", "one", "all", "wrap70", "exact100", "exact101", "both", "trunc_none", "write_between", "nan_inf", "random")


def run(tracker, steps, conv=lambda x: x, user_calls=0, info=False):
    """Feeds a script; returns the list of (timestep, dict) writes.  ``conv`` moves an array to where the tracker wants it.
    ``user_calls``: how many of the first steps of every write interval call ``track`` on the three USER_TAGS;
    ``info``: ``track_vector`` with a 16-float vector every step."""
    writes = []
    g = np.random.default_rng(123)
    calls = 0
    for t, (rew, term, trunc) in enumerate(steps):
        tracker.step(conv(rew), conv(term), None if trunc is None else conv(trunc))
        if calls < user_calls:
            calls += 1
            vals = g.standard_normal(3).astype(np.float32)
            for tag, v in zip(USER_TAGS, vals):
                tracker.track(tag, float(v))
        if info:
            tracker.track_vector(INFO_TAGS, conv(g.standard_normal(16).astype(np.float32)))
        data = tracker.post_interaction(t)
        if data is not None:
            writes.append((t + 1, data))
            calls = 0
    return writes


def same(a, b) -> bool:
    """Equal, NaN matching NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        return bool(np.array_equal(a, b, equal_nan=True))
    return bool(np.array_equal(a, b))


def same_writes(wa, wb) -> bool:
    if len(wa) != len(wb):
        return False
    for (ta, da), (tb, db) in zip(wa, wb):
        if ta != tb or list(da) != list(db):
            return False
        for k in da:
            if not same(da[k], db[k]):
                return False
    return True


# ---------------------------------------------------------------------------------------------------------------- edge scripts
# More than 65 536 envs: tracker_commit_kernel's 256 threads take the chunks t, t + 256, ... so chunks 256 and 257 belong to a second
# pass.  Twelve steps at most, so that the CPU specification stays in seconds.
BIG_SIZES = (65537, 65536 + 257)
MANY_TAGS = (300, 4096)


@functools.lru_cache(maxsize=None)
def big_script(n: int):
    """(steps, write_interval = 4) for n in BIG_SIZES.
    Interval 1: the step maximum (50) and minimum (-60) lie in the last chunk; at step 3 envs of chunk 0, of chunk 255 and of the
    last chunks (256, and 257 where n has one) finish together.
    Interval 2: a NaN reward in the last env at step 5; at step 6 more than 100 envs finish, the last env among them and, at
    n = 65 793, all of them beyond env 65 536, so only the 100 highest reach the rings.
    Interval 3: a +inf reward in the last chunk at step 9, finishers in chunks 0 and 256 at step 10."""
    assert n in BIG_SIZES
    rew, term, trunc = _blank(n, 12, 12)
    rew[0, n - 1], rew[2, 65536] = 50.0, -60.0
    first = [5, 200, 255 * 256 + 17, 65536, n - 1]
    term[3, first[:3]] = 1
    trunc[3, first[3:]] = 1
    rew[5, n - 1] = np.nan
    many = np.arange(65537, n, 2)[:130] if n > 65536 + 200 else np.arange(65400, 65536, 1)
    many = np.union1d(many, [n - 1])
    assert len(many) > 100 and (n <= 65536 + 200 or many.min() > 65536)
    term[6, many] = 1
    rew[9, 65536] = np.inf
    term[10, [3, 65536]] = 1
    trunc[10, 70] = 1
    return [(rew[t], term[t], trunc[t]) for t in range(12)], 4


def many_tags(count: int):
    """``count`` distinct tags: every third a (max), every third a (min), the others means."""
    return tuple(f"Stat / s{i}" + (" (max)", " (min)", "")[i % 3] for i in range(count))
