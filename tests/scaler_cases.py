"""What the running scaler's edge tests share (not a test module): tests/test_scaler.py, tests/test_gpu_scaler_edges.py and
tests/test_gpu_offpolicy_scaled_edges.py.

``ordered_train``   include/rover_scaler.h's "Reduction order" 1 to 4 and the merge restated in float64 numpy, one numpy operation per
                    device operation.  The library is built with -ffp-contract=off, so every float64 operation of the four launches
                    is one correctly rounded add, subtract, multiply or divide, and the block is predicted bit for bit.  Written
                    from the header, not from the kernel.
``exact_train``     the same update in exact rational arithmetic (``fractions``): the high-precision value.
``hard_columns``    columns a two-pass float64 variance finds hard, with matching start blocks.
``edge_block`` / ``edge_rows``   block values a resumed checkpoint can hold ((float)var 0, subnormal, FLT_MAX, inf ...) and input
                    rows for them.
``torch_forward`` ... ``numpy_inverse``   the fp32 oracle of both transforms on the CPU, written twice.

``python tests/scaler_cases.py`` prints the margins kept in profiles/scaler_edges_margins.txt.
"""
import functools
from fractions import Fraction

import numpy as np
import torch

FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)
U = 2.0 ** -52
CHUNK = 64                                   # rows per chunk
WAVES = 4                                    # strided partials per chunk
HPARAMS = ((1e-8, 5.0), (0.0, 5.0), (1e-8, float("inf")), (1e-3, 1.5))       # (eps, clip)


# ------------------------------------------------------------------------------------------------------------ the documented order
def _chunk_sums(v: np.ndarray) -> np.ndarray:
    """Order 1 (and 3): v (rows, w) float64 -> (n_chunks, w).  Partial q of a chunk adds its rows q, q + 4, ... in ascending order
    onto 0.0; the four combine as (p0 + p1) + (p2 + p3)."""
    rows, w = v.shape
    out = np.empty((-(-rows // CHUNK), w), np.float64)
    for k in range(out.shape[0]):
        c = v[CHUNK * k:CHUNK * (k + 1)]
        p = []
        for q in range(WAVES):
            s = np.zeros(w, np.float64)
            for r in range(q, c.shape[0], WAVES):
                s = s + c[r]
            p.append(s)
        out[k] = (p[0] + p[1]) + (p[2] + p[3])
    return out


def _ascending(parts: np.ndarray) -> np.ndarray:
    """Orders 2 and 4: the chunk sums in ascending chunk order onto 0.0."""
    s = np.zeros(parts.shape[1], np.float64)
    for k in range(parts.shape[0]):
        s = s + parts[k]
    return s


def ordered_batch(x_rows: np.ndarray):
    """(batch mean, unbiased batch variance) of float32 rows in the header's order."""
    x = np.asarray(x_rows)
    assert x.dtype == np.float32 and x.ndim == 2 and x.shape[0] >= 2
    rows = x.shape[0]
    with np.errstate(all="ignore"):
        xd = x.astype(np.float64)
        bmean = _ascending(_chunk_sums(xd)) / np.float64(rows)
        d = xd - bmean
        bvar = _ascending(_chunk_sums(d * d)) / np.float64(rows - 1)
    return bmean, bvar


def ordered_train(block: np.ndarray, x_rows: np.ndarray) -> np.ndarray:
    """The block (float64 ``mean[w], var[w], count``) after ``rover_scaler_train`` on the rows ``x_rows`` (float32, already gathered
    in idx order).  The merge is C's left-to-right evaluation of the header's expressions."""
    block = np.asarray(block, np.float64)
    rows, w = x_rows.shape
    assert block.shape == (2 * w + 1,)
    mean, var, cnt = block[:w], block[w:2 * w], block[2 * w]
    bmean, bvar = ordered_batch(x_rows)
    bc = np.float64(rows)
    with np.errstate(all="ignore"):
        tot = cnt + bc
        delta = bmean - mean
        m2 = ((var * cnt) + (bvar * bc)) + ((((delta * delta) * cnt) * bc) / tot)
        new_mean = mean + ((delta * bc) / tot)
        new_var = m2 / tot
    return np.concatenate([new_mean, new_var, [tot]])


def exact_train(block: np.ndarray, x_rows: np.ndarray):
    """The same update without rounding: (mean, var, count) as lists of ``Fraction`` (finite inputs only)."""
    block = np.asarray(block, np.float64)
    rows, w = x_rows.shape
    cnt, bc = Fraction(float(block[2 * w])), Fraction(rows)
    tot = cnt + bc
    means, variances = [], []
    for c in range(w):
        col = [Fraction(float(v)) for v in x_rows[:, c]]
        bm = sum(col) / bc
        bv = sum((v - bm) ** 2 for v in col) / (bc - 1)
        mean, var = Fraction(float(block[c])), Fraction(float(block[w + c]))
        delta = bm - mean
        variances.append((var * cnt + bv * bc + delta * delta * cnt * bc / tot) / tot)
        means.append(mean + delta * bc / tot)
    return means, variances, tot


def rel_err(got: float, want: Fraction) -> float:
    """|got - want| / |want| with the difference taken exactly; 0 / 0 is 0, x / 0 is inf."""
    diff = abs(Fraction(float(got)) - want)
    if want == 0:
        return 0.0 if diff == 0 else float("inf")
    return float(diff / abs(want))


# ------------------------------------------------------------------------------------------------------------------- hard columns
# (offset, sd); sd None: a constant column
HARD = ((1e6, 1e-2), (1e4, 1e-3), (0.0, 1e-20), (0.0, 1e18), (-3e7, 1.0), (2.0 ** 24, 1.0), (float(np.float32(0.1)), None), (2.5, None),
        (0.0, None), (1e-30, 1e-30), (0.5, 2.0))
HARD_NAMES = ("1e6 sd 1e-2", "1e4 sd 1e-3", "0 sd 1e-20", "0 sd 1e18", "-3e7 sd 1", "2^24 sd 1", "const 0.1f", "const 2.5", "const 0",
              "1e-30 sd 1e-30", "0.5 sd 2")
HARD_CONSTANT = tuple(i for i, (_, sd) in enumerate(HARD) if sd is None)
# err <= HARD_BOUND_CONSTANT * (|offset| / sd + 1) * 2**-52.  Proposed as 64; the worst ratio measured is 0.98 (the column 0 sd 1e18),
# so it is 4: a fourfold margin over the measurement (profiles/scaler_edges_margins.txt)
HARD_BOUND_CONSTANT = 4.0


def hard_columns(rows: int, seed: int, w: int = len(HARD)):
    """(x, start block with count 1e4, start block with count 2**40): x is (rows, w) float32, column i of kind HARD[i % 11] drawn as
    offset + sd * randn in float64 and rounded to float32 (at offset 1e6 a float32 ulp is 0.0625: the column is nearly constant,
    which is part of what makes it hard); the blocks hold mean = (float)offset, var = sd**2 (0 for a constant)."""
    g = np.random.default_rng(seed)
    kinds = [HARD[i % len(HARD)] for i in range(w)]
    x = np.empty((rows, w), np.float32)
    for i, (off, sd) in enumerate(kinds):
        x[:, i] = (off + (0.0 if sd is None else sd) * g.standard_normal(rows)).astype(np.float32)
    mean = np.array([np.float32(off) for off, _ in kinds], np.float64)
    var = np.array([0.0 if sd is None else sd * sd for _, sd in kinds], np.float64)
    return x, np.concatenate([mean, var, [1e4]]), np.concatenate([mean, var, [2.0 ** 40]])


def initial_block(w: int) -> np.ndarray:
    return np.concatenate([np.zeros(w), np.ones(w), [1.0]])


@functools.lru_cache(maxsize=None)
def hard_margins(rows_list=(2, 65, 257, 1027), seed=5):
    """Per column: the worst relative error of ``ordered_train`` against ``exact_train`` over the three start blocks and
    ``rows_list``, as (mean error, variance error, variance error / ((|offset| / sd + 1) * 2**-52)); for a constant column the
    third entry is the worst batch variance over (rows * 2**-52 * |c|)**2 instead."""
    w = len(HARD)
    worst = [[0.0, 0.0, 0.0] for _ in range(w)]
    for rows in rows_list:
        x, b1, b2 = hard_columns(rows, seed + rows)
        _, bvar = ordered_batch(x)
        for start in (initial_block(w), b1, b2):
            got = ordered_train(start, x)
            em, ev, _ = exact_train(start, x)
            for c, (off, sd) in enumerate(HARD):
                m, v = rel_err(got[c], em[c]), rel_err(got[w + c], ev[c])
                worst[c][0], worst[c][1] = max(worst[c][0], m), max(worst[c][1], v)
                if sd is None:
                    lim = (rows * U * abs(off)) ** 2
                    ratio = 0.0 if bvar[c] == 0.0 else (float("inf") if lim == 0.0 else float(bvar[c]) / lim)
                else:
                    ratio = max(m, v) / ((abs(off) / sd + 1.0) * U)
                worst[c][2] = max(worst[c][2], ratio)
    return worst


# ------------------------------------------------------------------------------------------------------- edge blocks and edge rows
EDGE_VAR = (0.0, 1e-50, 1e-46, 1e-40, FLT_MIN, 1e-20, 1.0, 1e30, FLT_MAX, 3.5e38, 1e39, 4.0)
EDGE_MEAN = (0.0, 1e-40, -1e-46, 1.0, FLT_MAX, 1e39, -1e39, 0.1, -0.0, 16777217.0, 2.5, 1e-45)


def edge_block(w: int) -> np.ndarray:
    """Column c holds variance EDGE_VAR[c % 12] and mean EDGE_MEAN[(c + c // 12) % 12]: at w = 12 the two lists side by side, at a
    larger width every variance meets other means as well.  count 1e4."""
    c = np.arange(w)
    mean = np.array(EDGE_MEAN, np.float64)[(c + c // 12) % 12]
    var = np.array(EDGE_VAR, np.float64)[c % 12]
    return np.concatenate([mean, var, [1e4]])


def edge_rows(w: int, seed: int = 0) -> np.ndarray:
    """(17, w) float32: zeros, the float32 means, +inf, -inf, NaN, 1e-40, 3.4e38, -3.4e38, 1e-45, then eight random rows (scale 3,
    1e30 and 1e-38)."""
    g = np.random.default_rng(1000 + 7 * w + seed)
    with np.errstate(over="ignore"):
        mean32 = edge_block(w)[:w].astype(np.float32)
    fixed = [np.zeros(w, np.float32), mean32]
    fixed += [np.full(w, v, np.float32) for v in (np.inf, -np.inf, np.nan, 1e-40, 3.4e38, -3.4e38, 1e-45)]
    rnd = [(g.standard_normal(w) * s).astype(np.float32) for s in (3.0, 3.0, 3.0, 3.0, 1e30, 1e30, 1e-38, 1e-38)]
    return np.stack(fixed + rnd)


# ----------------------------------------------------------------------------------------------------------------- the fp32 oracle
def torch_sanitise(x: torch.Tensor) -> torch.Tensor:
    return torch.nan_to_num(x, nan=0.0, posinf=FLT_MAX, neginf=0.0)


def torch_forward(x: torch.Tensor, blk: torch.Tensor, w: int, eps: float = 1e-8, clip: float = 5.0) -> torch.Tensor:
    """tests/test_gpu_scaler.py's expression, on CPU tensors."""
    mean, var = blk[:w], blk[w:2 * w]
    return torch.clamp((x - mean.float()) / (torch.sqrt(var.float()) + eps), min=-clip, max=clip)


def torch_inverse(x: torch.Tensor, blk: torch.Tensor, w: int, clip: float = 5.0) -> torch.Tensor:
    mean, var = blk[:w], blk[w:2 * w]
    return torch.sqrt(var.float()) * torch.clamp(x, min=-clip, max=clip) + mean.float()


def _clamp32(v, clip):
    lo, hi = np.float32(-clip), np.float32(clip)
    return np.where(v < lo, lo, np.where(v > hi, hi, v)).astype(np.float32)      # NaN passes both comparisons


def numpy_sanitise(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, np.float32)
    return np.where(np.isnan(x) | (x == -np.inf), np.float32(0.0), np.where(x == np.inf, np.float32(FLT_MAX), x)).astype(np.float32)


def numpy_forward(x: np.ndarray, blk: np.ndarray, w: int, eps: float = 1e-8, clip: float = 5.0) -> np.ndarray:
    """The header's forward expression, every operation in float32."""
    with np.errstate(all="ignore"):
        mu, sd = blk[:w].astype(np.float32), np.sqrt(blk[w:2 * w].astype(np.float32))
        den = sd + np.float32(eps)
        return _clamp32((np.asarray(x, np.float32) - mu) / den, clip)


def numpy_inverse(x: np.ndarray, blk: np.ndarray, w: int, clip: float = 5.0) -> np.ndarray:
    with np.errstate(all="ignore"):
        mu, sd = blk[:w].astype(np.float32), np.sqrt(blk[w:2 * w].astype(np.float32))
        return (sd * _clamp32(np.asarray(x, np.float32), clip)) + mu


def same_bits32(a: np.ndarray, b: np.ndarray) -> bool:
    """float32 arrays: NaN at the same places (whatever its payload), every other element equal on the bits."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb)) and bool(np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb]))


def same_bits64(a: np.ndarray, b: np.ndarray) -> bool:
    """float64 arrays, as ``same_bits32``."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb)) and bool(np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb]))


def margins_text() -> str:
    lines = ["column            worst rel err mean   worst rel err var   ratio"]
    for name, (m, v, r) in zip(HARD_NAMES, hard_margins()):
        lines.append(f"{name:<16}  {m:<19.3e}  {v:<18.3e}  {r:.3e}")
    return "\n".join(lines)


if __name__ == "__main__":
    print(margins_text())
