"""Fused TRPO update on the MI355X at its edges: row counts that cut the kernels' tiles short (16-row MFMA tiles, 64-row dense
blocks, 256-row head blocks, 2048-row weight-gradient chunks, more than 256 head blocks), value minibatches up to the production
4096 rows and past them, the value Adam across updates, the CG early stop, a line search that accepts a later trial, degenerate
settings, log_std exactly on a clamp bound, and a workspace that grows between ``policy_grad`` and ``fvp``.

The yardstick is test_gpu_trpo_update's: the float64 torch spec (isaac_rover_orbit_amd.trpo), and a fused result whose error
against it is at most 4x torch fp32's on the same inputs, plus a floor (trpo_helpers._check).  Control-flow choices (CG stop,
accepted trial) are asserted to lie clear of their thresholds on the float64 spec first, so that a fragile input fails loudly
instead of flaking."""
import math

import pytest
import torch

from trpo_helpers import DEV, _check, _copy, _err, _flat_to_sd, _nets, _rollout, _spec_step, _trainer

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32


def _surrogate_grads(pol, obs, act, logp, adv):
    """{dtype: ({name: dL/dparam}, L)} of the spec's surrogate in float64 and float32."""
    from isaac_rover_orbit_amd.trpo import surrogate_loss
    out = {}
    for dt in (F64, F32):
        p = _copy(pol, dt)
        loss = surrogate_loss(p, obs.to(dt), act.to(dt), logp.to(dt), adv.to(dt))
        gr = torch.autograd.grad(loss, list(p.parameters()))
        out[dt] = (dict(zip([k for k, _ in p.named_parameters()], gr)), float(loss))
    return out


def _fvp_refs(pol, obs, vsd, damping=0.1):
    from isaac_rover_orbit_amd.trpo import fisher_vector_product
    out = {}
    for dt in (F64, F32):
        p = _copy(pol, dt)
        v = torch.cat([vsd[k].reshape(-1) for k, _ in p.named_parameters()]).to(DEV, dt)
        out[dt] = _flat_to_sd(p, fisher_vector_product(p, obs.to(dt), v, damping).detach())
    return out


def _direction(pol, seed):
    gen = torch.Generator().manual_seed(seed)
    return {k: torch.randn(p.shape, generator=gen) for k, p in pol.named_parameters()}


def _cg_trace(pol, obs, act, logp, adv):
    """r.r after each of 10 iterations of the float64 spec's CG (no early stop) on the surrogate gradient."""
    from isaac_rover_orbit_amd.trpo import HPARAMS, conjugate_gradient, fisher_vector_product
    ref = _surrogate_grads(pol, obs, act, logp, adv)
    p64 = _copy(pol, F64)
    g64 = torch.cat([ref[F64][0][k].reshape(-1) for k, _ in p64.named_parameters()])
    trace = []
    conjugate_gradient(lambda v: fisher_vector_product(p64, obs.double(), v, HPARAMS["damping"]), g64, 10, 0.0, trace)
    return trace


def _cg_gap(trace):
    """(k, cg_tol): the first k in 2 .. 5 at which the float64 r.r falls 4x below every earlier r.r, and the geometric mean of
    the two, so that a CG stopped by cg_tol runs exactly k iterations with a 2x margin either side."""
    for k in range(2, 6):                                       # trace[j - 1] = r.r after iteration j
        above, below = min(trace[:k - 1]), trace[k - 1]
        if above >= 4.0 * below:
            return k, math.sqrt(above * below)
    pytest.fail(f"no 4x gap in the float64 CG residuals at iterations 2 .. 5: {trace}")


def _kink_free(net, obs, idx, margin=1e-5):
    """Mask of the rows of obs[idx] whose float64 pre-activations all lie at least ``margin`` from the LeakyReLU kink.  A pre-activation
    within fp32 rounding of 0 may take either slope in any fp32 forward (the kernels' or torch's); the row's gradient through
    that unit then moves by 99 %, which compares rounding at a branch, not the kernels."""
    net64, pre = _copy(net, F64), []
    lin = [m for m in net64.modules() if isinstance(m, torch.nn.Linear)]
    for m in lin[:-1]:                                          # the output layer has no kink
        m.register_forward_hook(lambda m, i, o: pre.append(o.detach()))
    with torch.no_grad():
        net64(obs[idx].double())
    ok = torch.ones(idx.numel(), dtype=torch.bool, device=idx.device)
    for z in pre:
        ok &= (z.abs() >= margin).all(1)
    return ok


def _replicas_match(tr):
    return torch.equal(tr.rep_p.view(tr.n_copies, tr.n_p), tr.params[:tr.n_p].expand(tr.n_copies, tr.n_p))


# ---------------------------------------------------------------------------------------------------------------- policy side
@pytest.mark.parametrize("B", [1, 17, 63, 257, 2049, 4097, 70001])
def test_policy_grad_and_fvp_at_ragged_rows(B):
    """B = 70001: 274 head blocks (reduce_rows' second stride) and 35 weight-gradient chunks, the last one ragged."""
    pol, val = _nets(10)
    obs, act, logp, ret, adv = _rollout(pol, B, seed=11)
    tr = _trainer(pol, val)
    tr.grad.fill_(float("nan"))                                 # every float of g is written
    g = tr.policy_grad(obs, act, logp, adv).clone()
    assert not torch.isnan(g).any()
    assert torch.count_nonzero(g[tr.n_p:tr.n_p + tr.n_v]) == 0
    ref = _surrogate_grads(pol, obs, act, logp, adv)
    _check(tr.unvector(g), ref[F64][0], ref[F32][0])
    assert tr.stats()["loss_old"] == pytest.approx(ref[F64][1], rel=1e-4, abs=1e-6)
    for j in range(2):
        vsd = _direction(pol, 100 * B + j)
        out = tr.fvp(obs, tr.vector(vsd), out=torch.full_like(tr.params, float("nan")))
        assert not torch.isnan(out).any() and torch.count_nonzero(out[tr.n_p:tr.n_p + tr.n_v]) == 0
        fr = _fvp_refs(pol, obs, vsd)
        _check(tr.unvector(out), fr[F64], fr[F32])


@pytest.mark.parametrize("B", [2049, 70001])
def test_policy_step_at_ragged_rows(B):
    """test_policy_step_matches_spec at ragged B, plus the replicas of the policy block bit for bit.  CG stops in a wide gap
    of the float64 residuals (_cg_gap): the default cg_tol of 1e-10 stops it early at these sizes too, but there fp32 and
    float64 residuals have parted, and the CG count would compare rounding rather than the kernels."""
    pol, val = _nets(12)
    obs, act, logp, ret, adv = _rollout(pol, B, seed=13)
    k, tol = _cg_gap(_cg_trace(pol, obs, act, logp, adv))
    tr = _trainer(pol, val, cg_tol=tol)
    g_out, x_out = torch.empty_like(tr.params), torch.empty_like(tr.params)
    tr.policy_step(obs, act, logp, adv, grad_out=g_out, dir_out=x_out)
    s = tr.stats()
    p64, st64 = _spec_step(pol, val, obs, act, logp, adv, F64, cg_residual_tolerance=tol)
    p32, st32 = _spec_step(pol, val, obs, act, logp, adv, F32, cg_residual_tolerance=tol)
    _check(tr.unvector(g_out), _flat_to_sd(p64, st64["grad"]), _flat_to_sd(p32, st32["grad"]))
    _check(tr.unvector(x_out), _flat_to_sd(p64, st64["direction"]), _flat_to_sd(p32, st32["direction"]), floor=1e-3)
    assert s["cg_iters"] == st64["cg_iters"] == k
    assert s["xhx"] == pytest.approx(st64["xhx"], rel=1e-3) and s["step"] == pytest.approx(st64["step"], rel=1e-3)
    assert s["accepted"] == st64["accepted"] >= 0
    assert s["kl"] == pytest.approx(st64["kl"], rel=2e-2) and s["loss_old"] == pytest.approx(st64["loss_old"], rel=1e-4, abs=1e-6)
    sd = tr.state_dict()["policy"]
    for key, ref in p64.state_dict().items():
        assert _err(sd[key], ref) <= 1e-3 * float(ref.norm()) + 1e-6, key
    assert _replicas_match(tr)


# ---------------------------------------------------------------------------------------------------------------- value side
@pytest.fixture(scope="module")
def value_buffer():
    """A 60 x 4096-row rollout buffer (obs, ret): the production size minibatch rows are gathered from."""
    g = torch.Generator(device=DEV).manual_seed(30)
    obs = torch.randn(60 * 4096, 965, device=DEV, generator=g) * 0.5
    ret = torch.randn(60 * 4096, device=DEV, generator=g)
    return obs, ret


@pytest.mark.parametrize("n", [1, 17, 2047, 2048, 2049, 4096, 4097])
def test_value_minibatch_at_ragged_and_production_rows(n, value_buffer):
    """Gradient and loss of a minibatch of n rows (2048: one weight-gradient chunk, 4096: the production two) against float64,
    rows drawn clear of the LeakyReLU kink (_kink_free); the policy block of grad untouched; and the workspace growth this
    first value minibatch causes leaves the theta_old cache of a preceding policy_grad intact: fvp returns the same bits
    before and after."""
    from isaac_rover_orbit_amd.ppo import unpack
    big_obs, big_ret = value_buffer
    rows = big_obs.shape[0]
    pol, val = _nets(14)
    obs, act, logp, _, adv = _rollout(pol, 257, seed=15)
    tr = _trainer(pol, val)
    tr.policy_grad(obs, act, logp, adv)
    v = tr.vector(_direction(pol, 16))
    fvp_before = tr.fvp(obs, v).clone()
    g_before = tr.grad.clone()
    gen = torch.Generator(device=DEV).manual_seed(n)
    cand = torch.cat([torch.randint(0, rows, (n + n // 4 + 8,), device=DEV, generator=gen),
                      torch.tensor([rows - 1], device=DEV)])
    ok = _kink_free(val, big_obs, cand)
    assert ok[-1] and int(ok[:-1].sum()) >= n, int(ok.sum())
    idx = cand[:-1][ok[:-1]][:n].contiguous()
    idx[-1] = rows - 1                                          # the very last row of the buffer
    if n > 2:
        idx[1] = idx[0]                                         # a repeat
    tr.value_minibatch(big_obs, big_ret, idx)
    assert torch.equal(tr.grad[:tr.n_p], g_before[:tr.n_p]) and torch.equal(tr.grad[tr.n_p + tr.n_v:], g_before[tr.n_p + tr.n_v:])
    g_sd = unpack(tr.desc_v, tr.grad[tr.n_p:tr.n_p + tr.n_v].clone())
    ref, loss64 = {}, None
    for dt in (F64, F32):
        vn = _copy(val, dt)
        loss = torch.nn.functional.mse_loss(big_ret[idx].to(dt), vn(big_obs[idx].to(dt)).squeeze(1))
        loss.backward()
        ref[dt] = {k: p.grad.clone() for k, p in vn.named_parameters()}
        if dt == F64:
            loss64 = float(loss)
    _check(g_sd, ref[F64], ref[F32])
    s = tr.stats()
    assert s["value_batches"] == 1 and s["value_loss_sum"] == pytest.approx(loss64, rel=1e-5)
    assert torch.equal(tr.fvp(obs, v), fvp_before)


def test_value_adam_across_two_updates():
    """trpo_reset_kernel keeps value_step: two updates of 2 epochs x 3 minibatches (B = 3 x 683) take 12 Adam steps, and the
    value network tracks the float64 spec on the same permutations element by element."""
    from isaac_rover_orbit_amd.trpo import HPARAMS, TorchTRPO
    pol, val = _nets(17)
    B = 3 * 683
    obs, act, logp, ret, adv = _rollout(pol, B, seed=18)
    torch.manual_seed(19)
    perms = [[torch.randperm(B, device=DEV) for _ in range(2)] for _ in range(2)]
    tr = _trainer(pol, val, epochs=2, minibatches=3)
    spec = TorchTRPO(_copy(pol, F64), _copy(val, F64), learning_epochs=2, mini_batches=3)
    for u in range(2):
        st = tr.update(obs, act, logp, ret, adv, perms=perms[u])
        ref = spec.update(obs.double(), act.double(), logp.double(), ret.double(), adv.double(), perms=perms[u])
        assert st["value_loss"] == pytest.approx(ref["value_loss"], rel=1e-4)
    s = tr.stats()
    assert s["value_step"] == 12 and s["value_batches"] == 6
    new = tr.state_dict()["value"]
    for k, p in spec.value.named_parameters():
        # twelve Adam steps move every weight by up to ~12 lr; agreement to 1 % of lr per element
        assert float((new[k].double() - p.detach().cpu()).abs().max()) <= 1e-2 * HPARAMS["value_learning_rate"], k
    x = obs[:64].contiguous()
    from isaac_rover_orbit_amd.policy import RoverNet
    assert torch.equal(tr.critic(x), RoverNet.from_state_dict(new, final_act="none")(x))


# ---------------------------------------------------------------------------------------------------------------- CG and search
def test_cg_stops_early_at_the_tolerance():
    """A cg_tol that the float64 spec's r.r crosses at iteration k in 2 .. 5 with a 2x margin on either side: the fused CG
    stops after k iterations (cg_done), below the tolerance, with the spec's direction at that tolerance."""
    pol, val = _nets(20)
    B = 4097
    obs, act, logp, ret, adv = _rollout(pol, B, seed=21)
    trace = _cg_trace(pol, obs, act, logp, adv)
    k, tol = _cg_gap(trace)
    tr = _trainer(pol, val, cg_tol=tol)
    x_out = torch.empty_like(tr.params)
    tr.policy_step(obs, act, logp, adv, dir_out=x_out)
    s = tr.stats()
    p64, st64 = _spec_step(pol, val, obs, act, logp, adv, F64, cg_residual_tolerance=tol)
    p32, st32 = _spec_step(pol, val, obs, act, logp, adv, F32, cg_residual_tolerance=tol)
    assert st64["cg_iters"] == k and s["cg_iters"] == k, (k, st64["cg_iters"], s["cg_iters"], trace)
    assert s["rr"] < tol
    _check(tr.unvector(x_out), _flat_to_sd(p64, st64["direction"]), _flat_to_sd(p32, st32["direction"]), floor=1e-3)


def test_line_search_accepts_a_later_trial(monkeypatch):
    """step_fraction > 1 overshoots the KL bound, and skrl's cumulative expected *= alpha then holds the improvement ratio down:
    the spec accepts a trial >= 2 with every trial's KL and ratio at least 5 % from their thresholds.  The fused search accepts
    the same trial after as many trials, with expected = g.full x prod alpha_i."""
    from isaac_rover_orbit_amd import trpo
    record, real = {}, trpo.line_search

    def traced(params_old, full_step, expected_improvement, evaluate, loss_old, max_kl, accept_ratio, step_fraction=1.0,
               max_backtrack_steps=10):
        trials = []

        def ev(theta):
            kl, loss = evaluate(theta)
            trials.append((float(kl), float(loss)))
            return kl, loss
        out = real(params_old, full_step, expected_improvement, ev, loss_old, max_kl, accept_ratio, step_fraction,
                   max_backtrack_steps)
        record.update(trials=trials, e0=float(expected_improvement), loss_old=float(loss_old), max_kl=max_kl,
                      accept_ratio=accept_ratio)
        return out

    monkeypatch.setattr(trpo, "line_search", traced)

    def clear(sf):
        """Every trial of the last spec search lies at least 5 % from both thresholds (expected *= alpha_i cumulatively)."""
        e = record["e0"]
        for i, (kl, loss) in enumerate(record["trials"]):
            e *= sf * 0.5 ** i
            ratio = (loss - record["loss_old"]) / e
            if abs(kl / record["max_kl"] - 1) < 0.05 or abs(ratio / record["accept_ratio"] - 1) < 0.05:
                return False
        return True

    chosen = None
    for seed in (20, 22, 24):                                   # the first rollout and step_fraction that give a clear case
        pol, val = _nets(seed)
        obs, act, logp, ret, adv = _rollout(pol, 4097, seed=seed + 1)
        for sf in (6.0, 5.0, 8.0, 12.0):
            p64, st64 = _spec_step(pol, val, obs, act, logp, adv, F64, step_fraction=sf)
            if st64["accepted"] >= 2 and clear(sf):
                chosen = (sf, p64, st64, dict(record))
                break
        if chosen:
            break
    assert chosen is not None, "no rollout / step_fraction gives a clear accepted trial >= 2 on the float64 spec"
    sf, p64, st64, rec = chosen
    expected = rec["e0"]
    for i in range(len(rec["trials"])):
        expected *= sf * 0.5 ** i
    tr = _trainer(pol, val, step_fraction=sf)
    tr.policy_step(obs, act, logp, adv)
    s = tr.stats()
    assert s["accepted"] == st64["accepted"] and s["trials"] == len(rec["trials"]) == st64["accepted"] + 1
    assert s["expected"] == pytest.approx(expected, rel=1e-3)
    sd = tr.state_dict()["policy"]
    for k, ref in p64.state_dict().items():
        assert _err(sd[k], ref) <= 1e-3 * float(ref.norm()) + 1e-6, k
    assert _replicas_match(tr)


@pytest.mark.parametrize("hp", [dict(cg_steps=0), dict(max_backtrack=0)])
def test_degenerate_settings_restore_theta_old(hp):
    """cg_steps = 0: x = 0, xHx = 0, step = inf, full = NaN, every trial fails; max_backtrack = 0: no trial.  Both restore
    theta_old and its replicas bit for bit, keep NaN out of params and leave the value block alone, as the spec does."""
    pol, val = _nets(24)
    obs, act, logp, ret, adv = _rollout(pol, 257, seed=25)
    tr = _trainer(pol, val, **hp)
    before = (tr.params.clone(), tr.rep_p.clone(), tr.rep_v.clone())
    tr.policy_step(obs, act, logp, adv)
    s = tr.stats()
    assert s["accepted"] == -1 and s["trials"] == tr.hp.max_backtrack
    if tr.hp.cg_steps == 0:
        assert s["cg_iters"] == 0 and s["xhx"] == 0.0 and math.isinf(s["step"])
    assert not torch.isnan(tr.params).any()
    assert torch.equal(tr.params, before[0]) and torch.equal(tr.rep_p, before[1]) and torch.equal(tr.rep_v, before[2])
    assert torch.equal(tr.params[tr.n_p:tr.n_p + tr.n_v], before[0][tr.n_p:tr.n_p + tr.n_v])
    names = dict(cg_steps="conjugate_gradient_steps", max_backtrack="max_backtrack_steps")
    _, st64 = _spec_step(pol, val, obs, act, logp, adv, F64, **{names[k]: v for k, v in hp.items()})
    assert st64["accepted"] == -1


@pytest.mark.parametrize("bound", ["max", "min"])
def test_log_std_on_a_clamp_bound(bound, monkeypatch):
    """log_std exactly on a clamp bound is inside the clamp (torch's clamp backward is inclusive): a non-zero gradient that
    matches float64, and (2 + damping) v on that log_std entry of F v.  The lower bound is moved to -1 (at -20, sigma = 2e-9
    is below the fp32 resolution of an action): the spec's clamp reads the module's HPARAMS."""
    from isaac_rover_orbit_amd import trpo
    kw, log_std = {}, (2.0, 0.3)
    if bound == "min":
        monkeypatch.setitem(trpo.HPARAMS, "log_std_min", -1.0)
        kw, log_std = dict(log_std_min=-1.0), (-1.0, 0.3)
    pol, val = _nets(26, log_std)
    obs, act, logp, ret, adv = _rollout(pol, 4097, seed=27)
    tr = _trainer(pol, val, **kw)
    g = tr.unvector(tr.policy_grad(obs, act, logp, adv).clone())
    ref = _surrogate_grads(pol, obs, act, logp, adv)
    assert ref[F64][0]["log_std_parameter"][0] != 0.0
    assert g["log_std_parameter"][0] != 0.0
    _check(g, ref[F64][0], ref[F32][0])
    vsd = _direction(pol, 28)
    out = tr.unvector(tr.fvp(obs, tr.vector(vsd)))
    v0 = float(vsd["log_std_parameter"][0])
    assert float(out["log_std_parameter"][0]) == pytest.approx((2.0 + tr.hp.damping) * v0, rel=1e-6)
    fr = _fvp_refs(pol, obs, vsd, tr.hp.damping)
    _check(out, fr[F64], fr[F32])
