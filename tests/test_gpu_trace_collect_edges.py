"""The fused episode recorder (trace_collect.TraceCollector, csrc/trace_kernels.hip) at the branches tests/test_gpu_trace_collect.py
does not reach.  Files are compared on bytes with the specification (trace.EpisodeRecorder); the device state block (count, status,
rows, head, len, pending, descriptors) is compared word for word with the CPU model (TorchTraceCollector) driven by the same
calls, in front of every drain (trace_cases.Paired).  Case lists are those of tests/test_trace_collect.py (tests/trace_cases.py).

  * copy_span: rows of 17, 18, 20 and 24 bytes (wide, with 1-, 2-, 4- and 8-byte tails; 18 bytes alternate the source alignment by
    env), 4096 / 4097 / 4098 / 4100 bytes (one span and two), 16 and 8 bytes (narrow), in six dtypes; sixteen streams
  * sources with a pitch: a column slice as observation (7 and 965 wide), a reward of three columns, a row slice as extra
  * uint8 done flags of 1, 2 and 255
  * ST_DESC and ST_RING raised by a collector whose drain is held off, at the step the model raises them: no descriptor behind
    desc_cap, no row staged over a pending one, every canary intact, the drain names the cause
  * R = 2 (max_episode_rows = drain_interval = 1); the commit's count / rows carried over three 256-env chunks
  * the close paths; pieces of 63, 64 and 65 rows against the narrow gather; a side stream
"""
import numpy as np
import pytest
import torch

from trace_cases import (CARRY_KW, CARRY_PATTERNS, EXTRAS, OVERRUN, OVERRUN_KW, WIDTH_CASES, WIDTH_STEPS, Paired, assert_same_files,
                         assert_same_state, drive, drive_overrun, model_base, pitched_sources, uint8_done)

from isaac_rover_orbit_amd import trace_collect as TC
from isaac_rover_orbit_amd.trace import load_trace

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KW = dict(max_episode_rows=6, drain_interval=3, piece_rows=7, guard_bytes=64)


def _make(n, obs_dim=7, extras=EXTRAS, max_rows=40, **kw):
    """The collector with canaries behind every buffer, paired with the model."""
    args = dict(KW, **kw)

    def make(base):
        return Paired(TC.TraceCollector(base, n, obs_dim, 2, extras, max_rows=max_rows, device=DEV, **args),
                      TC.TorchTraceCollector(model_base(base), n, obs_dim, 2, extras, max_rows=max_rows, **args))
    return make


def _guards(pair, t):
    assert pair.col.guards_intact(), f"a canary changed at step {t}"


def _run(tmp_path, n, steps, p_done=0.15, max_ep=6, obs_dim=7, extras=EXTRAS, max_rows=None, make_kw=None, **kw):
    """Spec, collector and model side by side; the files of all three are equal, the state was compared before every drain and
    the canaries after every step."""
    max_rows = (40 if n <= 5 else 10_000) if max_rows is None else max_rows
    ref, pair, fr, fg = drive(_make(n, obs_dim, extras, max_rows, **(make_kw or {})), str(tmp_path), n, steps, p_done, max_ep,
                              obs_dim=obs_dim, extras=extras, max_rows=max_rows, device=DEV, hook=_guards, **kw)
    rows = assert_same_files(fr, fg)
    assert_same_files(fr, pair.model_files)
    assert pair.col.guards_intact() and pair.checks >= 1
    return pair, fr, fg, rows


# -------------------------------------------------------------------------------------------------------------- 1. row widths
@pytest.mark.parametrize("n", [5, 67])
@pytest.mark.parametrize("case", sorted(WIDTH_CASES))
def test_row_widths_and_dtypes(tmp_path, case, n):
    ex, steps = WIDTH_CASES[case], WIDTH_STEPS[n]
    pair, fr, fg, rows = _run(tmp_path, n, steps, extras=ex)
    assert sum(rows) == steps * n and pair.checks >= steps // 3
    assert len(pair.col.specs) == (16 if case == "sixteen_streams" else 4 + len(ex))
    d = load_trace(fg[0])
    for k, p in ex.items():
        assert d[k].dtype == np.dtype(p["dtype"]) and d[k].shape[1:] == tuple(p["shape"])


def test_a_thirteenth_extra_is_refused(tmp_path):
    ex = dict(WIDTH_CASES["sixteen_streams"], one_more={"shape": (1,), "dtype": np.float32})
    with pytest.raises(ValueError, match="at most 16"):
        TC.TraceCollector(str(tmp_path / "run"), 2, 7, 2, ex, device=DEV, **KW)


# -------------------------------------------------------------------------------------------------- 2. sources with a pitch
@pytest.mark.parametrize("obs_dim", [7, 965])
def test_sources_with_a_pitch(tmp_path, obs_dim):
    n = 5
    seen = {}

    def put(name, x, inner=pitched_sources(n, obs_dim, DEV)):
        y = inner(name, x)
        seen[name] = (tuple(y.shape), y.stride(0), y.is_contiguous())
        return y
    pair, fr, fg, rows = _run(tmp_path, n, 20, obs_dim=obs_dim, to_device=put)
    assert sum(rows) == 20 * n
    assert seen["obs"] == ((n, obs_dim), obs_dim + 40, False) and seen["rew"] == ((n, 3), 3, True) and seen["feat"][2]


# ----------------------------------------------------------------------------------------------------- 3. uint8 done flags
def test_uint8_done_flags(tmp_path):
    n = 67
    sent = []

    def put(name, x, inner=uint8_done(DEV)):
        y = inner(name, x)
        if name == "done":
            assert y.dtype == torch.uint8
            sent.append(y.cpu())
        return y
    pair, fr, fg, rows = _run(tmp_path, n, 20, p_done=0.3, to_device=put)
    assert sum(rows) == 20 * n
    assert set(torch.cat(sent).tolist()) == {0, 1, 2, 255}
    flags = np.concatenate([load_trace(f)["terminated"].view(np.uint8).ravel() for f in fg])
    assert set(flags.tolist()) == {0, 1}


# -------------------------------------------------------------------------------------- 4. ring and descriptor overrun
@pytest.mark.parametrize("n", [5, 257])
@pytest.mark.parametrize("kind", sorted(OVERRUN))
def test_overrun_with_the_drain_held_off(tmp_path, kind, n):
    """No fault is provoked: the kernels are specified to refuse these rows and descriptors, and every buffer has its canary."""
    col = TC.TraceCollector(str(tmp_path / "dev"), n, 7, 2, EXTRAS, max_rows=10_000, device=DEV, **OVERRUN_KW)
    model = TC.TorchTraceCollector(str(tmp_path / "model"), n, 7, 2, EXTRAS, max_rows=10_000, **OVERRUN_KW)
    seen = []

    def after(t, want):
        assert_same_state(col, model)
        status = int(col.state[TC.W_STATUS])
        seen.append(status)
        assert status == int(model.state[TC.W_STATUS]) == want, (t, status, want)
        assert col.guards_intact(), t                                                  # the state block's canary: nothing behind desc_cap
    drive_overrun([col, model], kind, n, after)
    first, bit = OVERRUN[kind]["first"], OVERRUN[kind]["bit"]
    assert seen == [0] * first + [bit] * (OVERRUN[kind]["steps"] - first)
    assert bit == {"desc": TC.ST_DESC, "ring": TC.ST_RING}[kind]
    for i, (a, b) in enumerate(zip(col.stage, model.stage)):                           # a refused row overwrote nothing
        assert torch.equal(a.cpu(), b), col.keys[i]
    assert int(col.state[TC.W_COUNT]) == (8 * n if kind == "desc" else 3 * n) > 0
    with pytest.raises(TC.TraceOverflowError, match=OVERRUN[kind]["match"]):
        col.drain()
    with pytest.raises(TC.TraceOverflowError, match=OVERRUN[kind]["match"]):
        model.drain()
    assert col.guards_intact()
    col.close()
    model.close()


# --------------------------------------------------------------------------------------------------- 5. smallest geometry
@pytest.mark.parametrize("n", [1, 257])
def test_smallest_geometry(tmp_path, n):
    pair, fr, fg, rows = _run(tmp_path, n, 6, p_done=1.0, max_ep=1, extras=None, max_rows=10_000,
                              make_kw=dict(max_episode_rows=1, drain_interval=1, piece_rows=1))
    assert pair.col.R == 2 and sum(rows) == 6 * n and pair.checks >= 6


# ------------------------------------------------------------------------------------------- 6. commit carry over chunks
@pytest.mark.parametrize("n", [513, 600])
@pytest.mark.parametrize("pattern", sorted(CARRY_PATTERNS))
def test_commit_carry_over_chunks(tmp_path, pattern, n):
    pair, fr, fg, rows = _run(tmp_path, n, 8, p_done=0.0, max_ep=8, extras=None, make_kw=CARRY_KW, done_fn=CARRY_PATTERNS[pattern],
                              force=False)
    assert sum(rows) == 8 * n and pair.checks >= 3


# ------------------------------------------------------------------------------------------------------------ 7. close paths
def test_close_paths(tmp_path):
    n = 67
    pair, fr, fg, rows = _run(tmp_path / "a", n, 5, p_done=0.0, force=False)           # every env holds an open episode
    assert rows == [5 * n]
    pair, fr, fg, rows = _run(tmp_path / "b", n, 3, p_done=0.0, done_fn=lambda t, n_: torch.full((n_,), t == 2), force=False)
    assert rows == [3 * n]
    names = [c[0] for c in pair.col.calls]
    last = len(names) - 1 - names[::-1].index("rover_trace_drained")
    assert names[last + 1:] == ["rover_trace_commit_all"] and "rover_trace_gather" in names[:last]   # nothing to commit: no gather
    calls = list(pair.col.calls)
    assert pair.close() == fg and pair.col.calls == calls                              # a second close does nothing
    assert assert_same_files(fr, fg) == [3 * n]


# ---------------------------------------------------------------------------------- 8. pieces against the narrow gather
@pytest.mark.parametrize("piece", [63, 64, 65])
def test_piece_sizes_around_a_wave_of_rows(tmp_path, piece):
    n = 67
    pair, fr, fg, rows = _run(tmp_path, n, 20, make_kw=dict(piece_rows=piece))
    assert sum(rows) == 20 * n


# ------------------------------------------------------------------------------------------------------------ 9. side stream
def test_side_stream(tmp_path):
    n, ex, steps = 5, WIDTH_CASES["sixteen_streams"], WIDTH_STEPS[5]
    pair, fr, fg, rows = _run(tmp_path / "default", n, steps, extras=ex)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        pair2, fr2, fg2, rows2 = _run(tmp_path / "side", n, steps, extras=ex)
    side.synchronize()
    assert rows2 == rows and sum(rows) == steps * n
    assert_same_files(fg, fg2)
