"""Shared plumbing of the lift rollout collector's tests (tests/test_lift_rollout.py on the specification,
tests/test_gpu_lift_rollout.py and tests/test_gpu_lift_rollout_edges.py on the kernels): the trainer with hand-written scaler blocks,
one ``rover_lift_rollout_act`` launch between sentinel guard rows, the float64 measures of eps / act / logp, and the edge-case lists
both sides run -- action widths, log-std windows, poisoned rows, ids at the top of their range, the record kernel's inputs -- so
that the CPU file and the GPU file cannot drift apart."""
import numpy as np
import torch

ULP = 2.0 ** -23
EPS_TOL = 2.05e-06                 # |eps - float64 Box-Muller|
ACT_ULPS = 4
TAG = 0x4C524F00
OBS = 36
LOG_STD = (0.0, -0.7, 0.3, 2.5, -21.0, 1.0, -3.0, 0.1)          # inside, above (2.5) and below (-21) the clamps [-20, 2]
LS_CLAMPED = np.clip(np.array(LOG_STD, dtype=np.float32).astype(np.float64), -20.0, 2.0)
GUARD, FILL = 16, 777.0
OUT_KEYS = ("obs", "mean", "val", "act", "env_act", "logp", "eps")
INF, NAN = float("inf"), float("nan")


def _biteq(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def same_bits_nan_aware(a, b):
    """NaN at the same places (whatever its payload) and every other element equal on the bits."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    x, y = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return bool(torch.equal(na, nb)) and bool(torch.equal(x[~na], y[~nb]))


def logp_tol(A):
    """DESIGN 16's per-width bound: 8 * 2**-23 of the scale at A = 2, half an ulp more per further column (A = 1 as A = 2)."""
    return (8 + (max(A, 2) - 2) / 2) * ULP


def lift_rows(n, seed=0):
    """(n, 36) rows on the CPU: N(1, 4**2), so standardised values pass +5 and -5."""
    return torch.randn(n, OBS, generator=torch.Generator().manual_seed(seed)) * 4.0 + 1.0


# ------------------------------------------------------------------------------------------------------- the trainer, one launch
def scaler_blocks(seed=3):
    """(state block, value block) as float64 arrays: means of +-3 and in (-1, 1), variances in (0.25, 4), column 7 variance 0."""
    rng = np.random.RandomState(seed)
    mean = rng.uniform(-1.0, 1.0, OBS)
    mean[::5] = 3.0
    mean[2::5] = -3.0
    var = rng.uniform(0.25, 4.0, OBS)
    var[7] = 0.0                                                  # (o - mean) / (0 + 1e-8): +-5 after the clamp, 0 when o == mean
    return np.concatenate([mean, var, [100.0]]), np.array([-1.5, 4.0, 50.0])


def _make_trainer(seed=3, **kw):
    from isaac_rover_orbit_amd import lift_ppo as LP
    torch.manual_seed(seed)
    policy, value = LP.LiftMLP(LP.ACT_DIM, log_std=True), LP.LiftMLP(1)
    with torch.no_grad():
        policy.log_std_parameter.copy_(torch.tensor(LOG_STD))
    tr = LP.FusedLiftPPO(policy.state_dict(), value.state_dict(), lr=1e-3, **kw)
    state, value_blk = scaler_blocks(seed)
    tr.state_scaler.copy_(torch.from_numpy(state))
    tr.value_scaler.copy_(torch.from_numpy(value_blk))
    return tr


def _shapes(n, A):
    return {"obs": (n, OBS), "mean": (n, A), "val": (n, 1), "act": (n, A), "env_act": (n, A), "logp": (n,), "eps": (n, A)}


def hparams_of(**hp):
    from isaac_rover_orbit_amd import lift_rollout as LR
    h = LR.default_hparams()
    for k, v in hp.items():
        setattr(h, k, v)
    return h


def _run(tr, o, counter=0, outs=OUT_KEYS, value_scaler=True, log_std=None, **hp):
    """One launch; every output is the middle of a buffer with GUARD sentinel rows on both sides, which must come back untouched.
    ``tr``: anything with ``actor``, ``critic``, ``log_std``, ``state_scaler`` and ``value_scaler`` (a FusedLiftPPO, a WidthNets)."""
    from isaac_rover_orbit_amd import lift_rollout as LR
    n = o.shape[0]
    h = hparams_of(**hp)
    full = {k: torch.full((s[0] + 2 * GUARD,) + s[1:], FILL, device="cuda") for k, s in _shapes(n, tr.actor.out_dim).items()
            if k in outs or k in ("mean", "val")}
    view = {k: v[GUARD:GUARD + n] for k, v in full.items()}
    LR.lift_rollout_act(tr.actor, tr.critic, tr.log_std if log_std is None else log_std, o, counter, h, tr.state_scaler,
                        tr.value_scaler if value_scaler else None, **{k + "_out": view.get(k) for k in OUT_KEYS})
    torch.cuda.synchronize()
    for k, v in full.items():
        assert (v[:GUARD] == FILL).all() and (v[GUARD + n:] == FILL).all(), f"{k}: a guard row was written"
    return {k: v.clone() for k, v in view.items()}


def _errors(o, n, counter=0, seed=42, offset=0, ls=LS_CLAMPED):
    """(|eps - float64 spec|, act error / max(|mean|, |std eps|), logp error / sum_c (0.5 x_c**2 + |ls_c| + 0.919)) maxima over the
    rows of ``o`` (tensors on any device); ``ls``: the clamped log-std, one value per action column; ids are taken mod 2**32."""
    from isaac_rover_orbit_amd import rollout as R
    ls = np.asarray(ls, dtype=np.float64)
    eps64 = R.standard_normals(seed, offset + np.arange(n, dtype=np.int64), counter, ls.size, tag=TAG)
    eps, m, a = (o[k].cpu().numpy().astype(np.float64) for k in ("eps", "mean", "act"))
    noise = np.exp(ls) * eps
    d_act = np.abs(a - (m + noise)) / np.maximum(np.abs(m), np.abs(noise))
    x = (a - m) / np.exp(ls)
    want = (-0.5 * x * x - ls - 0.9189385332).sum(1)
    scale = (0.5 * x * x + np.abs(ls) + 0.919).sum(1)
    assert np.isfinite(want).all()
    d_lp = np.abs(o["logp"].cpu().numpy().astype(np.float64) - want) / scale
    return float(np.abs(eps - eps64).max()), float(d_act.max()), float(d_lp.max())


def check_sampling(o, n, ls, what, **kw):
    """Prints the three maxima of ``_errors`` and asserts them against EPS_TOL, 4 ulp and ``logp_tol(A)``; returns them."""
    A = np.asarray(ls).size
    d = _errors(o, n, ls=ls, **kw)
    print(f"{what}: |eps - spec| {d[0]:.3e} (bound {EPS_TOL:.3e}); act {d[1] / ULP:.2f} ulp ({ACT_ULPS}); "
          f"logp {d[2] / ULP:.2f} x 2**-23 of the scale ({logp_tol(A) / ULP:.1f})")
    assert d[0] <= EPS_TOL
    assert d[1] <= ACT_ULPS * ULP
    assert d[2] <= logp_tol(A)
    return d


# --------------------------------------------------------------------------------------------------------------- action widths
WIDTHS = (1, 2, 3, 7, 15, 16)
WIDTH_ROWS = (1, 15, 16, 17, 33)
MAX_WIDTH = 16
WIDTH_GAIN = 1.6                   # every layer's weights times this: the policy means of lift_rows come out O(1)


def log_std_of(A):
    """Distinct raw values per column; the last column above the upper clamp (2) and, from A = 2, column 0 below the lower (-20)."""
    ls = np.linspace(-1.5, 1.0, A)
    ls[A - 1] = 2.5
    if A > 1:
        ls[0] = -21.0
    assert len(set(ls.tolist())) == A
    return ls.astype(np.float32)


def width_state_dicts(A, seed=11):
    """(policy, value) LiftMLP state_dicts; the policy is the first A output rows of ONE 17-wide network, so the actor of width
    A + 1 is the actor of width A plus one appended output row."""
    from isaac_rover_orbit_amd import lift_ppo as LP
    torch.manual_seed(seed)
    wide, value = LP.LiftMLP(MAX_WIDTH + 1), LP.LiftMLP(1)
    out = []
    for net, rows in ((wide, A), (value, 1)):
        sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
        for k in sd:
            if k.endswith("weight"):
                sd[k] = sd[k] * WIDTH_GAIN
        sd["net.6.weight"], sd["net.6.bias"] = sd["net.6.weight"][:rows].clone(), sd["net.6.bias"][:rows].clone()
        out.append(sd)
    return out


class WidthNets:
    """What ``_run`` needs of a trainer, for an actor width a FusedLiftPPO does not take: ``lift_net`` networks of
    ``width_state_dicts(A)``, ``log_std_of(A)``, and the scaler blocks and ``standardize`` of ``trainer`` (they do not depend on A)."""

    def __init__(self, A, trainer, **kw):
        from isaac_rover_orbit_amd import lift_ppo as LP
        self.sd_p, self.sd_v = width_state_dicts(A)
        self.actor, self.critic = LP.lift_net(self.sd_p, **kw), LP.lift_net(self.sd_v, **kw)
        self.log_std = torch.from_numpy(log_std_of(A)).cuda()
        self.state_scaler, self.value_scaler, self.standardize, self.hp = trainer.state_scaler, trainer.value_scaler, trainer.standardize, trainer.hp


# ------------------------------------------------------------------------------------------------- float64 mean / val reference
BOUNDARY = 1e-6                    # rows with a standardised value (before the clamp) this close to +-clip are not compared
MAX_EXCLUDED = 0.05


def float64_forward(sd_p, sd_v, o, state_blk, value_blk, eps, clip):
    """(mean, val, near, nan) in float64 on the CPU: the header's formulas with every operation in float64 -- clamp((o - mean) /
    (sqrt(var) + eps), -clip, clip), ``net_forward`` on ``.double()`` weights, sqrt(var_v) * clamp(v, -clip, clip) + mean_v -- on
    the header's operands: the fp32 rows, (float)mean and (float)var of the blocks, the fp32 eps and clip.
    ``near`` marks the rows that are not compared: fp32 and float64 may clamp a value within BOUNDARY of +-clip (taken before the
    clamp: a state column, or the critic's output) on different sides.  ``nan`` marks the rows with a NaN standardised value, which
    have no float64 figure to be near to (the bit comparison with the trainer covers them, as a mask)."""
    from lift_ppo_reference import net_forward
    o, sb, vb = o.detach().double().cpu(), state_blk.detach().cpu().float().double(), value_blk.detach().cpu().float().double()
    clip = float(np.float32(clip))
    raw = (o - sb[:OBS]) / (sb[OBS:2 * OBS].sqrt() + float(np.float32(eps)))
    s = raw.clamp(-clip, clip)
    mean = net_forward({k: v.double() for k, v in sd_p.items()}, s)
    v = net_forward({k: v.double() for k, v in sd_v.items()}, s)
    val = vb[1].sqrt() * v.clamp(-clip, clip) + vb[0]
    near = ((raw.abs() - clip).abs() <= BOUNDARY).any(1) | ((v.abs() - clip).abs() <= BOUNDARY).any(1)
    return mean, val, near, torch.isnan(raw).any(1)


def check_float64(out, ref, what):
    """``out["mean"]`` / ``out["val"]`` against ``float64_forward``'s ``ref`` within 1e-5 * max(1, |ref|.max()), the bound of
    tests/test_gpu_lift_ppo.py::test_elu_forward_matches_float64, on the compared rows; at most MAX_EXCLUDED of the rows may be
    left out as near a clamp boundary."""
    mean, val, near, nan = ref
    assert float(near.double().mean()) <= MAX_EXCLUDED, (what, int(near.sum()), near.numel())
    keep = ~near & ~nan
    assert keep.any()
    for k, r in (("mean", mean), ("val", val)):
        r = r[keep]
        err = float((out[k].double().cpu()[keep] - r).abs().max())
        bound = 1e-5 * max(1.0, float(r.abs().max()))
        print(f"{what}: {k} against float64 {err:.3e} (bound {bound:.3e}; {int(near.sum())} of {near.numel()} rows near a clamp "
              f"boundary left out, {int(nan.sum())} NaN rows)")
        assert err <= bound, (what, k)


# ------------------------------------------------------------------------------------------------------------ log-std windows
WINDOWS = ((-1.0, 0.5), (0.3, 0.3))          # a window inside the default one, and min == max


# --------------------------------------------------------------------------------------------------------------- poisoned rows
POISON_ROWS = (16, 17, 33)
NAN_BITS = (0x7FC00123, 0xFFC00001)          # a quiet NaN with a payload, a negative one


def _poison_plan(n):
    plan = {0: ((3, NAN_BITS[0]), (10, INF)), 15: ((0, INF), (35, -INF)), 16: ((35, NAN_BITS[1]),)}
    plan[n - 1] = ((7, -INF), (20, INF))                           # the last row: infinities only (column 7 has variance 0)
    return {r: p for r, p in plan.items() if r < n}


def poison(o):
    """``o`` with NaN, +inf and -inf in chosen columns of rows {0, 15, 16, n - 1}: returns (rows, NaN rows, inf-only rows).  Row 0
    always has a NaN (and a +inf); the NaNs carry payloads, set on the bits."""
    p = o.clone()
    bits = p.view(torch.int32)
    nan_rows, inf_rows = [], []
    for r, cells in _poison_plan(o.shape[0]).items():
        for c, v in cells:
            if isinstance(v, int):
                bits[r, c] = v - (1 << 32) if v >= (1 << 31) else v
            else:
                p[r, c] = v
        (nan_rows if any(isinstance(v, int) for _, v in cells) else inf_rows).append(r)
    assert nan_rows and torch.isnan(p[nan_rows]).any(1).all() and not torch.isnan(p[inf_rows]).any()
    return p, sorted(nan_rows), sorted(inf_rows)


def check_poisoned(out, clean, raw, nan_rows, inf_rows, eps64):
    """What case 5 of the issue states, on the outputs ``out`` of the poisoned rows ``raw`` and ``clean`` of the same rows with the
    poisoned ones replaced by finite ones: obs bit-equal to the raw rows, NaN rows NaN in mean / val / act / env_act / logp with
    finite eps within its bound, inf-only rows finite, every other row of every output bit-equal to the clean run."""
    n = raw.shape[0]
    assert _biteq(out["obs"], raw)                                 # payloads kept
    for r in nan_rows:
        for k in ("mean", "val", "act", "env_act", "logp"):
            assert torch.isnan(out[k][r]).all(), (k, r)
        assert torch.isfinite(out["eps"][r]).all()
    for r in inf_rows:
        for k in ("mean", "val", "act", "env_act", "logp", "eps"):
            assert torch.isfinite(out[k][r]).all(), (k, r)
    assert float(np.abs(out["eps"].double().cpu().numpy() - eps64).max()) <= EPS_TOL
    others = [r for r in range(n) if r not in nan_rows and r not in inf_rows]
    for k in OUT_KEYS:
        assert _biteq(out[k][others], clean[k][others]), k
    assert _biteq(out["eps"], clean["eps"])                        # the draws do not depend on the rows at all


# ------------------------------------------------------------------------------------------ ids, seeds and counters at the top
WRAP_OFFSETS = (2 ** 31 - 1 - 16, 2 ** 31 - 1)                     # offset + row passes 2**31 inside one call of 33 rows
TOP_SEED, TOP_COUNTERS = 2 ** 64 - 1, (2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1)


# ----------------------------------------------------------------------------------------------------------- the record kernel
RECORD_NS = (1, 255, 256, 257)
RECORD_SCALES = (0.0, 1.0, -2.5)
FLAG_VALUES = (0, 1, 2, 255)
STILL_KS = (-1.0, 0.0, NAN)                                        # log[8] values under which the tally must not move


def record_inputs(n, seed):
    """(rew, terminated, truncated) on the CPU: rewards with NaN, +inf, -inf and -0.0 at every fourth place (all four also at
    n = 1 over seeds 0 .. 3), uint8 flags drawn from FLAG_VALUES."""
    rng = np.random.RandomState(1000 * n + seed)
    rew = rng.standard_normal(n).astype(np.float32)
    special = np.array([NAN, INF, -INF, -0.0], dtype=np.float32)
    at = np.arange(0, n, 4)
    rew[at] = special[(at // 4 + seed) % 4]
    flags = [np.array(FLAG_VALUES, dtype=np.uint8)[rng.randint(0, 4, n)] for _ in range(2)]
    return torch.from_numpy(rew), torch.from_numpy(flags[0]), torch.from_numpy(flags[1])


def expected_record(rew, term, trunc, scale):
    """(rew_out, done_out) by the header, in numpy fp32."""
    with np.errstate(invalid="ignore"):                              # inf * 0
        r = rew.numpy() * np.float32(scale)
    d = ((term.numpy() != 0) | (trunc.numpy() != 0)).astype(np.float32)
    return torch.from_numpy(r.astype(np.float32)), torch.from_numpy(d)


def record_log(k, seed, nan_at=None):
    log = torch.randn(16, generator=torch.Generator().manual_seed(seed))
    log[8] = k
    if nan_at is not None:
        log[nan_at] = NAN
    return log


def expected_tally(ep_sum, ep_count, log):
    """The header's tally in numpy fp32: if k > 0, ep_sum[j] += log[j] * (j < 6 ? k : 1) and ep_count += k; else nothing moves."""
    s, c, l = ep_sum.numpy().copy(), ep_count.numpy().copy(), log.numpy()
    k = l[8]
    if k > 0:
        w = np.where(np.arange(8) < 6, k, np.float32(1.0)).astype(np.float32)
        s = (s + l[0:8] * w).astype(np.float32)
        c = (c + k).astype(np.float32)
    return torch.from_numpy(np.asarray(s, dtype=np.float32)), torch.from_numpy(np.asarray(c, dtype=np.float32))
