"""The device recorder's CPU model (isaac_rover_orbit_amd.trace_collect.TorchTraceCollector) against the specification
(trace.EpisodeRecorder), bit for bit, and the error behaviour of its C ABI (include/rover_trace.h), on a host without a GPU.

  * the files are identical under ring wrap, pieces that cut episodes, file roll-over and partial episodes at close
  * ... with no env ever done, with every env done every step, and when nothing was appended
  * an explicit drain() in the middle of an interval changes nothing
  * an episode of max_episode_rows + 1 rows raises at the next drain; what was written before stays as it was
  * EpisodeRecorder's ValueErrors hold
  * every invalid argument of the C ABI returns ROVER_ERR_INVALID (1) and nothing is launched
  * device_bytes is the sum of what the class allocates
  * the edge cases of tests/test_gpu_trace_collect_edges.py (tests/trace_cases.py) on the model: row widths around 16 and 4096 bytes in
    every dtype, sixteen streams, pitched sources, uint8 flags of 2 and 255, ring and descriptor overrun with the drain held off,
    the smallest ring, the commit's carry over three chunks, the close paths and pieces around a wave of rows
"""
import ctypes as C

import numpy as np
import pytest
import torch

from trace_cases import (CARRY_KW, CARRY_PATTERNS, EXTRAS, OVERRUN, OVERRUN_KW, WIDTH_CASES, WIDTH_STEPS, Paired, assert_same_files,
                         assert_same_state, drive, drive_overrun, model_base, pitched_sources, uint8_done)

from isaac_rover_orbit_amd import trace_collect as TC
from isaac_rover_orbit_amd.trace import load_trace

KW = dict(max_episode_rows=6, drain_interval=3, piece_rows=7)


def _make(n, max_rows=40, extras=EXTRAS, obs_dim=7, **kw):
    args = dict(KW, **kw)
    return lambda base: TC.TorchTraceCollector(base, n, obs_dim, 2, extras, max_rows=max_rows, **args)


@pytest.mark.parametrize("n", [1, 5])
def test_model_equals_recorder(tmp_path, n):
    """40 steps at done-probability 0.15 with rings of 9 rows, pieces of 7 rows and files of 40 rows: the ring wraps, pieces cut
    episodes, and partial episodes are left at close; at n = 5 the 200 rows need several files."""
    ref, col, fr, fg = drive(_make(n), str(tmp_path), n, 40, 0.15, 6)
    steps = assert_same_files(fr, fg)
    assert sum(steps) == 40 * n
    if n == 5:
        assert len(fr) >= 5


@pytest.mark.parametrize("p_done", [0.0, 1.0])
def test_done_patterns(tmp_path, p_done):
    """Close only (the helper's time-out off: rings long enough for the 5 steps), and every env done at every step."""
    n = 5
    ref, col, fr, fg = drive(_make(n), str(tmp_path), n, 5 if p_done == 0.0 else 12, p_done, 6, force=False)
    steps = assert_same_files(fr, fg)
    assert sum(steps) == n * (5 if p_done == 0.0 else 12)


def test_close_straight_after_construction(tmp_path):
    ref, col, fr, fg = drive(_make(3), str(tmp_path), 3, 0, 0.0, 6)
    assert assert_same_files(fr, fg) == [0] and len(fg) == 1


def test_explicit_drain_changes_nothing(tmp_path):
    n = 5
    hook = lambda col, t: col.drain() if t in (0, 4, 5, 13) else None   # noqa: E731
    ref, col, fr, fg = drive(_make(n), str(tmp_path / "a"), n, 40, 0.15, 6, hook=hook)
    assert_same_files(fr, fg)
    ref2, col2, fr2, fg2 = drive(_make(n), str(tmp_path / "b"), n, 40, 0.15, 6)
    assert_same_files(fg2, fg)


def test_overflow_raises_at_drain_and_keeps_what_was_written(tmp_path):
    """Env 1 is never done: its 7th row (max_episode_rows + 1) is refused and the status sticks; the other envs finish an episode
    every second step.  The drains after steps 3 and 6 wrote their episodes; the next drain raises, and close() leaves exactly
    those episodes in the file."""
    n = 5
    done_fn = lambda t, n_: torch.tensor([t % 2 == 1 and e != 1 for e in range(n_)])   # noqa: E731
    ref, col, _, _ = drive(_make(n, max_rows=500), str(tmp_path), n, 6, 0.0, 6, max_rows=500, done_fn=done_fn, force=False, close=False)
    g = torch.Generator().manual_seed(5)
    from trace_cases import step_tensors
    obs, act, rew, info = step_tensors(g, n, 7, 2, EXTRAS)
    col.append(obs, act, rew, torch.zeros(n, dtype=torch.bool), info)                  # env 1: row 7
    with pytest.raises(TC.TraceOverflowError, match="max_episode_rows"):
        col.drain()
    with pytest.raises(RuntimeError):
        col.append(obs, act, rew, torch.zeros(n, dtype=torch.bool), info)
    got = col.close()
    ref._close_file()                                                                  # the spec's file with what it wrote by step 6
    assert assert_same_files(ref.files, got) == [4 * 3 * 2]


def test_recorder_value_errors_hold(tmp_path):
    with pytest.raises(ValueError, match="extension"):
        TC.TorchTraceCollector(str(tmp_path / "run.h5"), 2, 7, 2, max_episode_rows=6)
    with pytest.raises(ValueError, match="extension"):
        TC.TorchTraceCollector(str(tmp_path / "run.npz"), 2, 7, 2, max_episode_rows=6)
    col = TC.TorchTraceCollector(str(tmp_path / "run"), 2, 7, 2, max_rows=4, max_episode_rows=6, drain_interval=3)
    g = torch.Generator().manual_seed(0)
    with pytest.raises(ValueError, match="does not fit"):
        for t in range(5):                                                             # one episode of 5 rows, files of 4
            col.append(torch.randn(2, 7, generator=g), torch.randn(2, 2, generator=g), torch.randn(2, generator=g),
                       torch.tensor([t == 4, False]))
        col.close()
    with pytest.raises(ValueError):
        TC.TorchTraceCollector(str(tmp_path / "x"), 2, 7, 2)                           # neither max_episode_rows nor an env

    class Cfg:
        max_episode_length = 11
    assert TC.TorchTraceCollector(str(tmp_path / "y"), 2, 7, 2, env=Cfg()).max_ep == 11


def test_arguments_are_validated(tmp_path):
    col = TC.TorchTraceCollector(str(tmp_path / "run"), 4, 7, 2, EXTRAS, **KW)
    g = torch.Generator().manual_seed(0)
    from trace_cases import step_tensors
    obs, act, rew, info = step_tensors(g, 4, 7, 2, EXTRAS)
    done = torch.zeros(4, dtype=torch.bool)
    bad = [(obs.double(), act, rew, done, info), (obs[:3], act, rew, done, info), (obs[:, :6], act, rew, done, info),
           (obs, act[:, :1], rew, done, info), (obs, act, rew.double(), done, info), (obs, act, rew, done.float(), info),
           (obs, act, rew, done[:3], info), (obs, act, rew, done, None), (obs, act, rew, done, {"feat": info["feat"]}),
           (obs, act, rew, done, dict(info, tag=info["tag"].float())), (obs, act, rew, done, dict(info, feat=info["feat"][:, :4])),
           (obs.repeat(1, 2)[:, ::2], act, rew, done, info)]
    for args in bad:
        with pytest.raises(ValueError):
            col.append(*args)
    flags = torch.tensor([[0], [0], [255], [0]], dtype=torch.uint8)                   # uint8 flags: any non-zero byte is "done"
    col.append({"policy": obs}, act, rew.reshape(4, 1), flags, info)                   # accepted forms
    files = col.close()
    d = load_trace(files[0])
    assert d["number_of_steps"] == 4 and d["terminated"].dtype == np.bool_
    assert d["terminated"].view(np.uint8).ravel().tolist() == [1, 0, 0, 0]           # env 2's episode first, stored as True = 1
    assert np.array_equal(d["observations"], obs[[2, 0, 1, 3]].numpy())
    assert d["feat"].shape == (4, 5, 2) and d["tag"].dtype == np.uint8
    with pytest.raises(RuntimeError):
        col.append(obs, act, rew, done, info)


def test_permuted_extra_is_recorded_in_logical_order(tmp_path):
    """``extras["depth"]`` of RoverEnvCamera is a permute(0, 2, 1) view: the dense block is staged, the drain permutes it back."""
    from isaac_rover_orbit_amd.trace import EpisodeRecorder
    n, ex = 3, {"depth": {"shape": (4, 3), "dtype": np.float32}}
    ref = EpisodeRecorder(str(tmp_path / "ref"), n, 7, 2, ex, max_rows=40)
    col = TC.TorchTraceCollector(str(tmp_path / "dev"), n, 7, 2, ex, max_rows=40, **dict(KW, max_episode_rows=8))
    g = torch.Generator().manual_seed(3)
    for t in range(8):
        obs, act, rew = torch.randn(n, 7, generator=g), torch.randn(n, 2, generator=g), torch.randn(n, generator=g)
        depth = torch.randn(n, 3, 4, generator=g).permute(0, 2, 1)
        done = torch.tensor([t % 3 == 2, t == 5, False])
        ref.append_to_buffer(obs, act, rew, done, {"depth": depth})
        col.append(obs, act, rew, done, {"depth": depth})
    fr, fg = ref.close(), col.close()
    a, b = load_trace(fr[0]), load_trace(fg[0])
    assert a["number_of_steps"] == b["number_of_steps"] == 24
    assert a["depth"].shape == b["depth"].shape == (24, 4, 3) and np.array_equal(a["depth"].view(np.uint8), b["depth"].view(np.uint8))


def test_abi_errors_are_codes():
    """Sizes agree with the Python mirror; NULL pointers, n <= 0, row_bytes <= 0, too many streams, R < max_episode_rows + 1 and
    every other invalid argument return ROVER_ERR_INVALID (1).  Nothing reaches the GPU: the checks come before any HIP call."""
    from isaac_rover_orbit_amd import _lib
    lib = _lib.load()
    assert lib.rover_trace_stream_bytes() == C.sizeof(_lib.TraceStream) == 56
    for rb, want in ((1, 4), (3, 4), (4, 4), (8, 8), (15, 16), (16, 16), (17, 32), (3860, 3872), (57600, 57600)):
        assert lib.rover_trace_stage_pitch(rb) == TC.stage_pitch(rb) == want
    assert lib.rover_trace_stage_pitch(0) == lib.rover_trace_stage_pitch(-4) == 0
    assert lib.rover_trace_stage_bytes(5, 9, 3860) == 5 * 9 * 3872
    assert lib.rover_trace_stage_bytes(0, 9, 4) == lib.rover_trace_stage_bytes(5, 0, 4) == lib.rover_trace_stage_bytes(5, 9, 0) == 0
    for n, cap in ((1, 4), (5, 20), (256, 1), (4096, 4096 * 65)):
        assert lib.rover_trace_state_bytes(n, cap) == TC.state_bytes(n, cap) and TC.state_bytes(n, cap) % 16 == 0
    assert lib.rover_trace_state_bytes(0, 4) == lib.rover_trace_state_bytes(4, 0) == 0

    # never dereferenced: every call below is refused before a launch
    SRC, STAGE, OUT, STATE, DONE = 0x10000, 0x2000000, 0x3000000, 0x4000000, 0x5000000

    def streams(k=2, **kw):
        arr = (_lib.TraceStream * max(k, 1))()
        for s in arr:
            s.src, s.src_pitch, s.stage, s.stage_pitch, s.out, s.out_pitch, s.row_bytes, s.flags = SRC, 3860, STAGE, 3872, OUT, 3860, 3860, 0
            for name, v in kw.items():
                setattr(s, name, v)
        return arr

    good = dict(st=streams(), k=2, state=STATE, n=16, R=10, max_ep=6, cap=64, done=DONE)

    def app(**kw):
        a = dict(good, **kw)
        return lib.rover_trace_append(a["st"], a["k"], a["state"], a["n"], a["R"], a["max_ep"], a["cap"], a["done"], None)

    assert lib.rover_trace_append(None, 0, None, 0, 0, 0, 0, None, None) == 1 and len(lib.rover_last_error()) > 0
    many = streams(17)
    for bad in (dict(st=None), dict(k=0), dict(k=-1), dict(st=many, k=17), dict(state=None), dict(state=STATE + 4), dict(n=0), dict(n=-2),
                dict(R=6), dict(R=5), dict(R=0), dict(max_ep=0), dict(max_ep=10), dict(cap=0), dict(done=None),
                dict(n=1 << 20, R=1 << 12), dict(st=streams(row_bytes=0)), dict(st=streams(row_bytes=-4)), dict(st=streams(src=None)),
                dict(st=streams(stage=None)), dict(st=streams(stage_pitch=3856)), dict(st=streams(src_pitch=3856)),
                dict(st=streams(flags=2)), dict(st=streams(flags=1))):
        assert app(**bad) == 1, bad
    assert app(R=6) == 1 and b"max_episode_rows + 1" in lib.rover_last_error()
    assert app(st=many, k=17) == 1 and b"ROVER_TRACE_MAX_STREAMS" in lib.rover_last_error()

    def gat(**kw):
        a = dict(dict(good, r0=0, rows=8), **kw)
        return lib.rover_trace_gather(a["st"], a["k"], a["state"], a["n"], a["R"], a["cap"], a["r0"], a["rows"], None)

    for bad in (dict(st=None), dict(k=0), dict(st=many, k=17), dict(state=None), dict(n=0), dict(R=1), dict(cap=0), dict(r0=-1), dict(rows=0),
                dict(rows=-3), dict(r0=2 ** 31 - 4, rows=8), dict(st=streams(out=None)), dict(st=streams(stage=None)),
                dict(st=streams(out_pitch=100)), dict(st=streams(row_bytes=0))):
        assert gat(**bad) == 1, bad
    assert lib.rover_trace_init(None, 4, 4, None) == 1 and lib.rover_trace_init(STATE, 0, 4, None) == 1
    assert lib.rover_trace_init(STATE, 4, 0, None) == 1 and lib.rover_trace_init(STATE + 8, 4, 4, None) == 1
    assert lib.rover_trace_commit_all(None, 4, 10, 8, None) == 1 and lib.rover_trace_commit_all(STATE, 0, 10, 8, None) == 1
    assert lib.rover_trace_commit_all(STATE, 4, 1, 8, None) == 1 and lib.rover_trace_commit_all(STATE, 4, 10, 0, None) == 1
    assert lib.rover_trace_drained(None, 4, None) == 1 and lib.rover_trace_drained(STATE, 0, None) == 1
    if not torch.cuda.is_available():
        with pytest.raises(_lib.RoverHipError):
            TC.TraceCollector("unused", 4, 7, 2, max_episode_rows=6)                   # the product path fails loudly, no CPU fallback


@pytest.mark.parametrize("extras,piece", [(None, None), (EXTRAS, 7), ({"depth": {"shape": (160, 90), "dtype": np.float32}}, None)])
def test_device_bytes_is_what_is_allocated(tmp_path, extras, piece):
    n, obs_dim = 5, 965
    col = TC.TorchTraceCollector(str(tmp_path / "run"), n, obs_dim, 2, extras, max_episode_rows=6, drain_interval=3, piece_rows=piece)
    want = TC.TraceCollector.device_bytes(n, obs_dim, 2, extras, max_episode_rows=6, drain_interval=3, piece_rows=piece)
    tensors = [col.state] + col.stage + col.out
    assert want == sum(t.numel() * t.element_size() for t in tensors) == col.allocated_bytes()
    rows = [3860, 8, 4, 1] + ([4 * int(np.prod(p["shape"])) if p["dtype"] == np.float32 else int(np.prod(p["shape"])) for p in (extras or {}).values()])
    assert sum(t.numel() for t in col.stage) == n * 9 * sum(TC.stage_pitch(r) for r in rows)
    col.close()
    # sizing a run: 750-row episodes at 4096 envs take 3.9 KB per env step without extras, 61.5 KB with the depth image
    per_row = TC.TraceCollector.device_bytes(4096, 965, 2, None, 750, 64) / (4096 * 814)
    assert 3884 <= per_row < 3950


# ------------------------------------------------------------------------------- the edge cases the GPU runs, on the model
@pytest.mark.parametrize("n", [5, 67])
@pytest.mark.parametrize("case", sorted(WIDTH_CASES))
def test_row_widths_and_dtypes(tmp_path, case, n):
    """Rows of 16, 17, 18, 20, 24 and 8 bytes, of 4096, 4097, 4098 and 4100 bytes, in uint8, int16, float16, float32, float64 and
    int64; twelve extras are sixteen streams.  A second model runs behind ``Paired``: the state comparison itself is rehearsed."""
    ex, max_rows, steps = WIDTH_CASES[case], 40 if n == 5 else 1000, WIDTH_STEPS[n]

    def make(base):
        return Paired(_make(n, max_rows, ex)(base), _make(n, max_rows, ex)(model_base(base)))
    ref, col, fr, fg = drive(make, str(tmp_path), n, steps, 0.15, 6, extras=ex, max_rows=max_rows)
    assert sum(assert_same_files(fr, fg)) == steps * n and col.checks >= steps // 3
    assert_same_files(fr, col.model_files)
    d = load_trace(fg[0])
    for k, p in ex.items():
        assert d[k].dtype == np.dtype(p["dtype"]) and d[k].shape[1:] == tuple(p["shape"])


def test_a_thirteenth_extra_is_refused(tmp_path):
    ex = dict(WIDTH_CASES["sixteen_streams"], one_more={"shape": (1,), "dtype": np.float32})
    with pytest.raises(ValueError, match="at most 16"):
        TC.TorchTraceCollector(str(tmp_path / "run"), 2, 7, 2, ex, **KW)


@pytest.mark.parametrize("obs_dim", [7, 965])
def test_sources_with_a_pitch(tmp_path, obs_dim):
    n = 5
    ref, col, fr, fg = drive(_make(n, obs_dim=obs_dim), str(tmp_path), n, 20, 0.15, 6, obs_dim=obs_dim, to_device=pitched_sources(n, obs_dim))
    assert sum(assert_same_files(fr, fg)) == 20 * n


def test_uint8_done_flags(tmp_path):
    n = 5
    ref, col, fr, fg = drive(_make(n), str(tmp_path), n, 20, 0.3, 6, to_device=uint8_done())
    assert sum(assert_same_files(fr, fg)) == 20 * n
    flags = np.concatenate([load_trace(f)["terminated"].view(np.uint8).ravel() for f in fg])
    assert set(flags.tolist()) == {0, 1}


@pytest.mark.parametrize("kind", sorted(OVERRUN))
def test_overrun_with_the_drain_held_off(tmp_path, kind):
    """The status bit appears at the step worked out in trace_cases.py and not before, nothing is written past desc_cap, a refused
    row does not overwrite a staged one, and the drain names what was overrun."""
    n = 5
    col = TC.TorchTraceCollector(str(tmp_path / "run"), n, 7, 2, EXTRAS, **OVERRUN_KW)
    snap = {}

    def after(t, want):
        assert int(col.state[TC.W_STATUS]) == want, (t, int(col.state[TC.W_STATUS]), want)
        assert col.guards_intact()
        if t == OVERRUN[kind]["first"] - 1:
            snap["stage"] = [s.clone() for s in col.stage]
    drive_overrun([col], kind, n, after)
    if kind == "ring":
        assert all(torch.equal(a, b) for a, b in zip(snap["stage"], col.stage))        # the refused rows changed nothing
        assert int(col.state[TC.W_COUNT]) == 3 * n and int(col.state[TC.W_ROWS]) == 9 * n
    else:
        assert int(col.state[TC.W_COUNT]) == 8 * n and int(col.state[TC.W_ROWS]) == 8 * n
    with pytest.raises(TC.TraceOverflowError, match=OVERRUN[kind]["match"]):
        col.drain()
    col.close()


@pytest.mark.parametrize("n", [1, 257])
def test_smallest_geometry(tmp_path, n):
    """max_episode_rows = 1, drain_interval = 1: rings of two rows, every env done at every step, pieces of one row."""
    kw = dict(max_episode_rows=1, drain_interval=1, piece_rows=1)
    ref, col, fr, fg = drive(_make(n, 1000, None, **kw), str(tmp_path), n, 6, 1.0, 1, extras=None, max_rows=1000)
    assert col.R == 2 and sum(assert_same_files(fr, fg)) == 6 * n


@pytest.mark.parametrize("n", [513, 600])
@pytest.mark.parametrize("pattern", sorted(CARRY_PATTERNS))
def test_commit_carry_over_chunks(tmp_path, pattern, n):
    ref, col, fr, fg = drive(_make(n, 10_000, None, **CARRY_KW), str(tmp_path), n, 8, 0.0, 8, extras=None, max_rows=10_000,
                             done_fn=CARRY_PATTERNS[pattern], force=False)
    assert sum(assert_same_files(fr, fg)) == 8 * n


def test_close_paths(tmp_path):
    n = 5
    # every env holds an open episode, two rows of it staged since the last drain
    ref, col, fr, fg = drive(_make(n), str(tmp_path / "a"), n, 5, 0.0, 6, force=False)
    assert assert_same_files(fr, fg) == [25]
    # every env done at step 2, where a drain runs: close() has nothing to commit
    ref, col, fr, fg = drive(_make(n), str(tmp_path / "b"), n, 3, 0.0, 6, done_fn=lambda t, n_: torch.full((n_,), t == 2), force=False)
    assert assert_same_files(fr, fg) == [15] and int(col.state[TC.W_COUNT]) == 0
    assert col.close() == fg                                                           # a second close changes nothing
    assert assert_same_files(fr, fg) == [15]


@pytest.mark.parametrize("piece", [63, 64, 65])
def test_piece_sizes_around_a_wave_of_rows(tmp_path, piece):
    n = 67
    ref, col, fr, fg = drive(_make(n, 1000, guard_bytes=64, piece_rows=piece), str(tmp_path), n, 20, 0.15, 6, max_rows=1000,
                             hook=lambda c, t: c.guards_intact() or pytest.fail("a canary changed"))
    assert sum(assert_same_files(fr, fg)) == 20 * n


def test_assert_same_state_sees_a_difference(tmp_path):
    """The helper the GPU tests lean on: equal for two models driven alike, and it fails on one changed word of each kind."""
    n = 5
    cols = [TC.TorchTraceCollector(str(tmp_path / f"run{i}"), n, 7, 2, EXTRAS, **OVERRUN_KW) for i in range(2)]
    g = torch.Generator().manual_seed(0)
    from trace_cases import step_tensors
    for t in range(2):
        obs, act, rew, info = step_tensors(g, n, 7, 2, EXTRAS)
        for c in cols:
            c.append(obs, act, rew, torch.arange(n) % 2 == t, info)
    assert_same_state(*cols)
    H, d0 = TC.HEADER_WORDS, TC.desc_word(n)
    assert int(cols[0].state[TC.W_COUNT]) == 5
    for word in (TC.W_COUNT, TC.W_STATUS, TC.W_ROWS, H + 1, H + n + 1, H + 2 * n + 1, d0 + 4 * 4 + 3):
        cols[1].state[word] += 1
        with pytest.raises(AssertionError):
            assert_same_state(*cols)
        cols[1].state[word] -= 1
    assert_same_state(*cols)
    cols[1].state[d0 + 4 * 5] += 1                                                     # behind the last descriptor: not compared
    assert_same_state(*cols)
    for c in cols:
        c.close()
