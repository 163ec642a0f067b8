"""Shared plumbing of the rollout-collector GPU tests (tests/test_gpu_rollout.py, tests/test_gpu_rollout_edges.py): inputs with
non-finite values at chosen places, one ``rover_rollout_act`` launch into freshly filled outputs, bit comparison."""
import numpy as np
import torch

from helpers import random_policy_weights, synthetic_obs

OUT_KEYS = ("obs", "mean", "val", "act", "env_act", "logp", "eps")


def _inject(rows, n):
    """Rows [0, n) with non-finite values on rows 0, 15, 16 and n - 1 (those that exist): -inf and NaN alternate over the first and
    the last encoder column (3, 963), column 0 and a mid-row column; +inf sits in column 964.  That column is in the row but read by
    neither network (models.py:95 drops the last ray), so the FLT_MAX it becomes is checked in obs_out without saturating the
    networks to inf - inf = NaN, for which no bound on act or logp could be stated."""
    raw = rows[:n].clone()
    vals = [float("-inf"), float("nan")]
    for i, r in enumerate(sorted({0, 15, 16, n - 1})):
        if r >= n:
            continue
        for j, c in enumerate((3, 963, 0, 500 + r % 7)):
            raw[r, c] = vals[(i + j) % 2]
        raw[r, 964] = float("inf")
    return raw


def _biteq(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _hp(**kw):
    from isaac_rover_orbit_amd import rollout as R
    hp = R.default_hparams()
    for k, v in kw.items():
        setattr(hp, k, v)
    return hp


def _run(nets, raw, log_std, counter=0, outs=("obs", "act", "env_act", "logp", "eps"), **hp):
    from isaac_rover_orbit_amd import rollout as R
    n, A = raw.shape[0], nets[0].out_dim
    f = dict(dtype=torch.float32, device="cuda")
    shapes = {"obs": (n, 965), "act": (n, A), "env_act": (n, A), "logp": (n,), "eps": (n, A)}
    o = {k: torch.full(shapes[k], 777.0, **f) for k in outs}
    mean, val = R.rollout_act(nets[0], nets[1], log_std, raw, counter, _hp(**hp), **{k + "_out": v for k, v in o.items()})
    o["mean"], o["val"] = mean, val
    torch.cuda.synchronize()
    return o


# ------------------------------------------------------------------------------------------------- inputs without a RoverEnv
def synthetic_rows(n, seed=0):
    """(n, 965) rows of ``helpers.synthetic_obs`` on the GPU, about one ray in sixteen a miss (-inf, as the scanner writes it)."""
    obs = synthetic_obs(n, seed=seed)
    miss = np.random.RandomState(seed + 1000).rand(n, 960) < 1.0 / 16.0
    obs[:, 4:964][miss] = -np.inf
    return torch.from_numpy(obs).cuda()


def actor_weights(A, seed=21):
    return random_policy_weights(seed=seed, out_dim=A, scale=3.0)


def make_nets(A, seed=21, extra_rows=0, **kw):
    """Actor (``A + extra_rows`` tanh outputs) and critic (one plain output) of the reference architecture.  ``extra_rows`` appends
    output rows to the last layer of the SAME weights, so columns [0, A) of the wider actor are those of the narrower one."""
    from isaac_rover_orbit_amd.policy import RoverNet
    wa, ba = actor_weights(A, seed)
    if extra_rows:
        rng = np.random.RandomState(seed + 500)
        wa = wa[:5] + [np.concatenate([wa[5], (rng.uniform(-1, 1, (extra_rows, 128)) / np.sqrt(128) * 3.0).astype(np.float32)])]
        ba = ba[:5] + [np.concatenate([ba[5], (rng.uniform(-1, 1, (extra_rows,)) / np.sqrt(128) * 3.0).astype(np.float32)])]
    wc, bc = random_policy_weights(seed=seed + 1, out_dim=1, scale=3.0)
    return RoverNet(wa, ba, n_enc=2, final_act="tanh", **kw), RoverNet(wc, bc, n_enc=2, final_act="none", **kw)


def shapes_of(n, A):
    return {"obs": (n, 965), "mean": (n, A), "val": (n, 1), "act": (n, A), "env_act": (n, A), "logp": (n,), "eps": (n, A)}


def run_into(nets, raw, log_std, o, counter=0, **hp):
    """One launch into the caller's tensors ``o`` (keys of OUT_KEYS; "mean" and "val" required, a missing key is passed as NULL)."""
    from isaac_rover_orbit_amd import rollout as R
    R.rollout_act(nets[0], nets[1], log_std, raw, counter, _hp(**hp), **{k + "_out": o.get(k) for k in OUT_KEYS})
    torch.cuda.synchronize()
    return o


def run_all(nets, raw, log_std, counter=0, **hp):
    """All seven outputs of one launch on fresh tensors of exactly n rows."""
    n, A = raw.shape[0], nets[0].out_dim
    o = {k: torch.full(s, 777.0, dtype=torch.float32, device="cuda") for k, s in shapes_of(n, A).items()}
    return run_into(nets, raw, log_std, o, counter, **hp)


def float64_errors(o, ls):
    """(act error / max(|mean|, |std eps|), logp error / sum_c (0.5 x_c**2 + |ls_c| + 0.919)) per element / row against float64
    on the returned eps, mean and act, ``ls`` the clamped log-std: the two measures of tests/test_gpu_rollout.py."""
    eps, m, a = (o[k].cpu().numpy().astype(np.float64) for k in ("eps", "mean", "act"))
    ls = np.asarray(ls, dtype=np.float64)
    noise = np.exp(ls) * eps
    d_act = np.abs(a - (m + noise)) / np.maximum(np.abs(m), np.abs(noise))
    x = (a - m) / np.exp(ls)
    want = (-0.5 * x * x - ls - 0.9189385332).sum(1)
    scale = (0.5 * x * x + np.abs(ls) + 0.919).sum(1)
    assert np.isfinite(want).all()
    d_lp = np.abs(o["logp"].cpu().numpy().astype(np.float64) - want) / scale
    return d_act, d_lp
