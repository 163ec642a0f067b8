"""Fused lift PPO update on the MI355X (include/rover_lift_train.h) at moved hyper-parameters and edges: every field of
rover_lift_ppo_hparams that a kernel reads is moved and seen to matter, clip + Adam and a three-step chain against float64, the
state words, row counts round the 4 / 16 / 64 / 256 / 4096 boundaries of the two reductions, repeated indices, a stale or
NaN-filled oversized workspace, the scaler entry at every width class of the C ABI, and every branch of the KL schedule.

Kernel against float64, throughout: err(fused, f64) <= 4 err(torch float32, f64) + 1e-6 |f64|, the float32 side being the SAME
reference function (tests/lift_ppo_reference.py) run with dtype=torch.float32 on the same inputs.  Every comparison prints both
errors.  Hyper-parameters reach the references as the float32 values the struct holds (a kernel cannot see more)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from lift_ppo_reference import NumpyScaler, clip_and_adam, loss_terms_and_grads, net_forward
from test_gpu_lift_ppo import DEV, _grads_of, _nets, _trainer

pytestmark = pytest.mark.gpu
LOG_STD = [-0.5, 0.2, 0.0, -1.0, 0.4, -0.2, 0.1, 2.5]
INVALID = 1                                                            # ROVER_ERR_INVALID


# ---------------------------------------------------------------------------------------------------------------- helpers
def _rule(tag, fused, t32, f64):
    """The tolerance rule; returns the bound.  Tensors (any device) or floats."""
    fused, t32, f64 = (x.detach().double().cpu() if torch.is_tensor(x) else torch.tensor(float(x), dtype=torch.float64)
                       for x in (fused, t32, f64))
    e_f = float((fused - f64).norm())
    e_t = float((t32 - f64).norm())
    ref = float(f64.norm())
    bound = 4 * e_t + 1e-6 * ref
    print(f"[lift-edges] {tag}: fused {e_f:.3e} float32 {e_t:.3e} |f64| {ref:.3e} ratio {e_f / max(e_t, 1e-300):.3f} "
          f"of-bound {e_f / max(bound, 1e-300):.3f}")
    assert e_f <= bound, (tag, e_f, e_t, ref)
    return bound


def _rollout(pol, val, B, seed, lp_noise, v_noise, ls_min=-20.0, ls_max=2.0, scale=1.0):
    """test_gpu_lift_ppo._rollout with the log_std clamp of the trainer under test, so that the ratios stay round 1."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    obs = torch.randn(B, 36, device=DEV, generator=g) * scale
    with torch.no_grad():
        s = torch.clamp(obs / (1.0 + 1e-8), -5.0, 5.0)                # the initial scaler: mean 0, var 1
        mean, v0 = pol(s), val(s)[:, 0]
        ls = pol.log_std_parameter.clamp(ls_min, ls_max)
        act = mean + ls.exp() * torch.randn(B, 8, device=DEV, generator=g)
        lp = (-0.5 * ((act - mean) / ls.exp()) ** 2 - ls - 0.9189385332).sum(-1)
    logp = (lp + lp_noise * torch.randn(B, device=DEV, generator=g)).contiguous()
    oldv = (v0 + v_noise * torch.randn(B, device=DEV, generator=g)).contiguous()
    ret = (oldv + torch.randn(B, device=DEV, generator=g)).contiguous()
    adv = torch.randn(B, device=DEV, generator=g)
    return obs.contiguous(), act.contiguous(), logp, oldv, ret, adv


@functools.lru_cache(maxsize=None)
def _world(lp_noise=0.3, v_noise=0.4, ls_min=-20.0, ls_max=2.0):
    """Networks and an 8192-row rollout, made once per setting and never written to."""
    pol, val = _nets(2, log_std=LOG_STD)
    return pol, val, _rollout(pol, val, 8192, 3, lp_noise, v_noise, ls_min, ls_max)


def _loss_kw(hp, **over):
    kw = dict(clip=hp.clip_ratio, vclip=hp.value_clip, vscale=hp.value_loss_scale, ls_min=hp.log_std_min, ls_max=hp.log_std_max)
    kw.update(over)
    return kw


def _flat(grads):
    return [(r, k, grads[r][k]) for r in ("policy", "value") for k in grads[r]]


def _check_minibatch(tag, tr, pol_sd, val_sd, args, stats):
    """Gradient per tensor and stats[0:3] of the minibatch just run, by the rule.  Returns (float64 grads, per-tensor bounds)."""
    kw = _loss_kw(tr.hp)
    _, kl, pl, vl, ref = loss_terms_and_grads(pol_sd, val_sd, *args, **kw)
    _, kl32, pl32, vl32, t32 = loss_terms_and_grads(pol_sd, val_sd, *args, dtype=torch.float32, **kw)
    fused = _grads_of(tr)
    bounds = {}
    for r, k, g64 in _flat(ref):
        bounds[r, k] = _rule(f"{tag} grad {r}.{k}", fused[r][k], t32[r][k], g64)
    st = stats.cpu()
    for i, (name, a32, a64) in enumerate((("kl", kl32, kl), ("policy_loss", pl32, pl), ("value_loss", vl32, vl))):
        _rule(f"{tag} stats[{i}] {name}", st[i], a32, a64)
    assert st[3].item() == 0.0
    ls = pol_sd["log_std_parameter"].cpu()
    g_ls = fused["policy"]["log_std_parameter"]
    outside = (ls < tr.hp.log_std_min) | (ls > tr.hp.log_std_max)
    assert torch.all(g_ls[outside] == 0.0) and torch.all(ref["policy"]["log_std_parameter"].cpu()[outside] == 0.0)
    return ref, bounds


# ------------------------------------------------------------------------------------- 1. moved loss hyper-parameters
ALL_MOVED = dict(clip_ratio=0.4, value_clip=0.05, value_loss_scale=7.0, log_std_min=-0.3, log_std_max=0.3)
LOSS_CASES = {
    "clip_ratio=0.05": (dict(clip_ratio=0.05), 0.3, 0.4),
    "clip_ratio=0.4": (dict(clip_ratio=0.4), 0.3, 0.4),
    "value_clip=0.05": (dict(value_clip=0.05), 0.3, 0.4),
    "value_clip=1.0": (dict(value_clip=1.0), 0.3, 0.7),
    "value_loss_scale=0.5": (dict(value_loss_scale=0.5), 0.3, 0.4),
    "value_loss_scale=7.0": (dict(value_loss_scale=7.0), 0.3, 0.4),
    "log_std=(-0.3,0.3)": (dict(log_std_min=-0.3, log_std_max=0.3), 0.3, 0.4),
    "all": (ALL_MOVED, 0.3, 0.4),
}


@pytest.mark.parametrize("case", list(LOSS_CASES))
def test_moved_loss_hyper_parameters_match_float64_and_matter(case):
    """4096 rows of 8192.  The coverage and the `discriminating` conditions are properties of the inputs, computed from the
    float64 reference alone: every clip branch holds more than 10 rows, and the float64 gradient at the moved value lies more
    than 100 bounds away from the one at the default value in at least one tensor (in the all-moved case: for every field put
    back on its own as well), so a kernel that ignores a field fails that tensor's comparison."""
    from isaac_rover_orbit_amd import lift_ppo as LP
    moved, lp_noise, v_noise = LOSS_CASES[case]
    dflt = LP.default_hparams()
    ls_min, ls_max = moved.get("log_std_min", dflt.log_std_min), moved.get("log_std_max", dflt.log_std_max)
    pol, val, (obs, act, logp, oldv, ret, adv) = _world(lp_noise, v_noise, ls_min, ls_max)
    tr = _trainer(pol, val, **moved)
    n = 4096
    idx = torch.randperm(8192, device=DEV, generator=torch.Generator(device=DEV).manual_seed(11))[:n].contiguous()
    stats = torch.full((4,), -7.0, device=DEV)
    tr.minibatch(obs, act, logp, oldv, ret, adv, idx, stats=stats)
    s = tr.standardize(obs[idx].contiguous(), "state")
    args = (s, act[idx], logp[idx], oldv[idx], ret[idx], adv[idx])
    psd, vsd = pol.state_dict(), val.state_dict()
    # coverage, from the float64 forward
    with torch.no_grad():
        P = {k: v.double() for k, v in psd.items()}
        ls = P["log_std_parameter"].clamp(tr.hp.log_std_min, tr.hp.log_std_max)
        lp = (-0.5 * ((act[idx].double() - net_forward(P, s.double())) / ls.exp()) ** 2 - ls - 0.9189385332).sum(-1)
        r = (lp - logp[idx].double()).exp()
        dv = net_forward({k: v.double() for k, v in vsd.items()}, s.double())[:, 0] - oldv[idx].double()
    a = adv[idx]
    for side in (r < 1 - tr.hp.clip_ratio, r > 1 + tr.hp.clip_ratio):
        assert int((side & (a > 0)).sum()) > 10 and int((side & (a < 0)).sum()) > 10
    assert int(((r >= 1 - tr.hp.clip_ratio) & (r <= 1 + tr.hp.clip_ratio)).sum()) > 10
    assert int((dv > tr.hp.value_clip).sum()) > 10 and int((dv < -tr.hp.value_clip).sum()) > 10
    assert int((dv.abs() <= tr.hp.value_clip).sum()) > 10
    ref, bounds = _check_minibatch(case, tr, psd, vsd, args, stats)
    g_ls = _grads_of(tr)["policy"]["log_std_parameter"]
    raw = torch.tensor(LOG_STD)
    inside = (raw >= tr.hp.log_std_min) & (raw <= tr.hp.log_std_max)
    assert int(inside.sum()) == (4 if "log_std_min" in moved else 7)
    assert torch.all(g_ls[inside] != 0.0) and torch.all(g_ls[~inside] == 0.0)
    # discriminating: the field(s) put back to the default move the float64 gradient by more than 100 bounds
    groups = [tuple(moved)] if len(moved) <= 2 else [("clip_ratio",), ("value_clip",), ("value_loss_scale",),
                                                     ("log_std_min", "log_std_max"), tuple(moved)]
    key_of = dict(clip_ratio="clip", value_clip="vclip", value_loss_scale="vscale", log_std_min="ls_min", log_std_max="ls_max")
    for fields in groups:
        back = {key_of[f]: getattr(dflt, f) for f in fields}
        other = loss_terms_and_grads(psd, vsd, *args, **_loss_kw(tr.hp, **back))[4]
        worst = max(float((other[r_][k].cpu() - g.cpu()).norm()) / bounds[r_, k] for r_, k, g in _flat(ref))
        print(f"[lift-edges] {case}: default {fields} moves the float64 gradient by {worst:.1f} bounds")
        assert worst > 100.0, (case, fields, worst)


# ------------------------------------------------------------------------------------- 2. clip + Adam against float64
def _packed_grad(p0, seed, norm):
    """A synthetic gradient of norm `norm`: in the trainer's flat layout (exact zeros on the padding) and per tensor, keyed and
    ordered as `p0` (the trainer's state_dict)."""
    from isaac_rover_orbit_amd import lift_ppo as LP
    g = torch.Generator().manual_seed(seed)
    gsd = {r: {k: torch.randn(p.shape, generator=g) * (0.05 if r == "policy" else 0.02) for k, p in p0[r].items()} for r in p0}
    tot = math.sqrt(sum(float(t.double().pow(2).sum()) for r in gsd for t in gsd[r].values()))
    gsd = {r: {k: (t * (norm / tot)).contiguous() for k, t in gsd[r].items()} for r in gsd}
    flat = np.concatenate([LP.pack(gsd["policy"])[1], LP.pack(gsd["value"])[1], gsd["policy"]["log_std_parameter"].numpy()])
    return torch.from_numpy(flat).to(DEV), gsd


def _sd_list(sd):
    return [sd[r][k] for r in ("policy", "value") for k in sd[r]]


def _padding_mask(tr):
    """True where the flat layout holds a padding float: pack all-ones networks."""
    from isaac_rover_orbit_amd import lift_ppo as LP
    sd = tr.state_dict()
    ones = [LP.pack({k: torch.ones_like(v) for k, v in sd[r].items() if k != LP.LOG_STD_KEY})[1] for r in ("policy", "value")]
    return torch.from_numpy(np.concatenate(ones + [np.ones(8, np.float32)]) == 0.0).to(DEV)


def _fword(tr, i):
    return np.float32(tr.state.view(torch.float32)[i].item())


def _within_one_ulp(a, b):
    return abs(np.float64(a) - np.float64(b)) <= np.spacing(np.float32(b))


def _change_err(now_list, p0, ref_list):
    """|| (now - p0) - (ref - p0) || over the whole vector, and || ref - p0 ||."""
    num = den = 0.0
    for now, start, ref in zip(now_list, _sd_list(p0), ref_list):
        d_ref = ref.double().cpu() - start.double()
        num += float(((now.double().cpu() - start.double()) - d_ref).norm()) ** 2
        den += float(d_ref.norm()) ** 2
    return num ** 0.5, den ** 0.5


def _change_rule(tag, sd_fused, p0, ref32, ref64):
    e_f, den = _change_err(_sd_list(sd_fused), p0, ref64)
    e_t, _ = _change_err(ref32, p0, ref64)
    print(f"[lift-edges] {tag}: fused {e_f:.3e} float32 {e_t:.3e} |f64| {den:.3e} ratio {e_f / max(e_t, 1e-300):.3f}")
    assert den > 0 and e_f <= 4 * e_t + 1e-6 * den, (tag, e_f, e_t, den)


APPLY_SETTINGS = {
    "a-clips": (dict(), 5.0),
    "b-free": (dict(), 0.1),
    "c-moved": (dict(max_grad_norm=0.25, beta1=0.8, beta2=0.99, eps=1e-5, lr=3e-3), 5.0),
}


@pytest.mark.parametrize("n_copies", [4, 1])
@pytest.mark.parametrize("setting", list(APPLY_SETTINGS))
def test_apply_matches_float64_clip_and_adam_and_writes_its_state(setting, n_copies):
    """Three apply() calls on synthetic gradients of norm 5 x (1, 1.3, 0.7) (0.1 x ... in the un-clipped setting) against
    clip_and_adam, the state words against the header's formulas, and `grad` left holding the clipped gradient."""
    from isaac_rover_orbit_amd import lift_ppo as LP
    kw, norm = APPLY_SETTINGS[setting]
    pol, val = _nets(5, log_std=LOG_STD)
    tr = _trainer(pol, val, n_copies=n_copies, **kw)
    hp, lr = tr.hp, tr.lr
    assert lr == kw.get("lr", 1e-4)
    p0 = {r: {k: v.clone() for k, v in sd.items()} for r, sd in tr.state_dict().items() if r in ("policy", "value")}
    chains = {}
    for dt in (torch.float64, torch.float32):
        ps = [t.to(dt) for t in _sd_list(p0)]
        chains[dt] = [ps, [torch.zeros_like(t) for t in ps], [torch.zeros_like(t) for t in ps]]
    for step, mult in ((1, 1.0), (2, 1.3), (3, 0.7)):
        gflat, gsd = _packed_grad(p0, 20 + step, norm * mult)
        tr.grad.copy_(gflat)
        tr.apply()
        out = {}
        for dt, (ps, m, v) in chains.items():
            ps, m, v, _, nrm, coef = clip_and_adam(ps, _sd_list(gsd), m, v, step, lr, hp.max_grad_norm, hp.beta1, hp.beta2, hp.eps, dt)
            chains[dt] = [ps, m, v]
            out[dt] = (nrm, coef)
        tag = f"apply {setting} copies {n_copies} step {step}"
        _change_rule(tag + " params", tr.state_dict(), p0, chains[torch.float32][0], chains[torch.float64][0])
        gn, coef = _fword(tr, 3), _fword(tr, 4)
        _rule(tag + " grad_norm", float(gn), out[torch.float32][0], out[torch.float64][0])
        assert coef == min(np.float32(1.0), np.float32(hp.max_grad_norm) / (gn + np.float32(1e-6)))
        assert (coef == 1.0) == (setting == "b-free") and (out[torch.float64][1] == 1.0) == (setting == "b-free")
        assert _within_one_ulp(_fword(tr, 5), np.float32(lr / (1.0 - float(hp.beta1) ** step)))
        assert _within_one_ulp(_fword(tr, 6), np.float32(math.sqrt(1.0 - float(hp.beta2) ** step)))
        assert tr.steps == step
        assert torch.equal(tr.grad, gflat * float(coef))               # the overwrite: grad holds the clipped gradient
        if setting == "b-free":
            assert torch.equal(tr.grad, gflat)
    pad = _padding_mask(tr)
    assert int(pad.sum()) > 0 and torch.all(gflat[pad] == 0)
    for t in (tr.params, tr.adam_m, tr.adam_v):
        assert torch.all(t[pad] == 0.0) and bool(torch.any(t[~pad] != 0.0))
    Pn, Vn = tr.n_p, tr.n_v
    assert tr.rep_p.numel() == n_copies * Pn and tr.rep_v.numel() == n_copies * Vn
    for c in range(n_copies):
        assert torch.equal(tr.rep_p[c * Pn:(c + 1) * Pn], tr.params[:Pn])
        assert torch.equal(tr.rep_v[c * Vn:(c + 1) * Vn], tr.params[Pn:Pn + Vn])
    rows = torch.randn(37, 36, device=DEV, generator=torch.Generator(device=DEV).manual_seed(6))
    sd = tr.state_dict()
    assert torch.equal(tr.actor(rows), LP.lift_net(sd["policy"])(rows)) and torch.equal(tr.critic(rows), LP.lift_net(sd["value"])(rows))
    assert not torch.equal(tr.actor(rows), LP.lift_net(pol.state_dict())(rows))


# ------------------------------------------------------------------------------------- 3. three chained steps, all moved
def test_three_chained_steps_with_everything_moved_track_the_float64_chain():
    """minibatch + apply three times (768 rows each) with every loss and optimiser hyper-parameter moved, against the chain
    float64 autograd gradient -> float64 clip_and_adam; the float32 baseline is the same chain in float32."""
    moved = dict(ALL_MOVED, max_grad_norm=0.25, beta1=0.8, beta2=0.99, eps=1e-5, lr=3e-3, kl_early_stop=0.0)
    pol, val, (obs, act, logp, oldv, ret, adv) = _world(0.3, 0.4, -0.3, 0.3)
    tr = _trainer(pol, val, **moved)
    hp, lr = tr.hp, tr.lr
    p0 = {r: {k: v.clone() for k, v in sd.items()} for r, sd in tr.state_dict().items() if r in ("policy", "value")}
    keys = [(r, k) for r in ("policy", "value") for k in p0[r]]
    perm = torch.randperm(8192, device=DEV, generator=torch.Generator(device=DEV).manual_seed(13))
    chains = {}
    for dt in (torch.float64, torch.float32):
        ps = [t.to(dt).to(DEV) for t in _sd_list(p0)]
        chains[dt] = [ps, [torch.zeros_like(t) for t in ps], [torch.zeros_like(t) for t in ps]]
    for step in (1, 2, 3):
        idx = perm[(step - 1) * 768:step * 768].contiguous()
        tr.minibatch(obs, act, logp, oldv, ret, adv, idx)
        tr.apply()
        s = tr.standardize(obs[idx].contiguous(), "state")
        args = (s, act[idx], logp[idx], oldv[idx], ret[idx], adv[idx])
        for dt, (ps, m, v) in chains.items():
            sd = {"policy": {}, "value": {}}
            for (r, k), t in zip(keys, ps):
                sd[r][k] = t
            g = loss_terms_and_grads(sd["policy"], sd["value"], *args, dtype=dt, **_loss_kw(hp))[4]
            ps, m, v, _, _, coef = clip_and_adam(ps, [g[r][k] for r, k in keys], m, v, step, lr, hp.max_grad_norm, hp.beta1, hp.beta2,
                                                 hp.eps, dt)
            chains[dt] = [ps, m, v]
            assert coef < 1.0
        assert tr.steps == step and tr._word(7) == 0
        _change_rule(f"chain step {step} params", tr.state_dict(), p0, chains[torch.float32][0], chains[torch.float64][0])


# ------------------------------------------------------------------------------------- 4. row-count edges and repeats
def _edge_idx(kind, n):
    g = torch.Generator(device=DEV).manual_seed(100 + n)
    if kind == "distinct":
        return torch.randperm(8192, device=DEV, generator=g)[:n].contiguous()
    if kind == "one-row":
        return torch.full((n,), 4321, dtype=torch.int64, device=DEV)
    pool = torch.randperm(8192, device=DEV, generator=g)[:10]
    idx = pool[torch.randint(0, 10, (n,), device=DEV, generator=g)].contiguous()
    assert idx.unique().numel() < n
    return idx


@pytest.mark.parametrize("kind,n", [("distinct", n) for n in (3, 4, 5, 15, 16, 63, 64, 65, 255, 256, 257, 4097)]
                         + [("one-row", 64), ("ten-rows", 100)])
def test_row_count_edges_and_repeated_indices(kind, n):
    """Gradient and stats by the rule, the forward's outputs bit-identical to the inference forward, at the row counts round the
    quad (4), workgroup (16), wave-group (64), stride (256) and wrap (4096) boundaries; repeats in idx are just rows.  Then the
    same with the minibatch's own scaler update from a non-trivial state, against NumpyScaler on the gathered float64 rows."""
    pol, val, (obs, act, logp, oldv, ret, adv) = _world()
    idx = _edge_idx(kind, n)
    psd, vsd = pol.state_dict(), val.state_dict()
    for train in (False, True):
        tr = _trainer(pol, val)
        tr.standardize((obs[:3000] * 2.5 + 0.7).contiguous(), "state", train=True)      # a non-trivial scaler state
        tr.standardize((obs[3000:3500] * 0.6 - 0.2).contiguous(), "state", train=True)
        blk0 = tr.state_scaler.clone()
        stats = torch.full((4,), -7.0, device=DEV)
        mean_out, value_out = torch.empty(n, 8, device=DEV), torch.empty(n, 1, device=DEV)
        tr.minibatch(obs, act, logp, oldv, ret, adv, idx, train_scaler=train, stats=stats, mean_out=mean_out, value_out=value_out)
        blk = tr.state_scaler.cpu().numpy()
        if train:
            ns = NumpyScaler(36)
            b0 = blk0.cpu().numpy()
            ns.mean, ns.var, ns.count = b0[:36].copy(), b0[36:72].copy(), float(b0[72])
            ns.train(obs[idx].double().cpu().numpy())
            np.testing.assert_allclose(blk[:36], ns.mean, rtol=1e-12)
            np.testing.assert_allclose(blk[36:72], ns.var, rtol=1e-12)
            assert blk[72] == ns.count == b0[72] + n
        else:
            assert torch.equal(tr.state_scaler, blk0)
        s = tr.standardize(obs[idx].contiguous(), "state")            # with the updated statistics
        assert torch.equal(mean_out, tr.actor(s)) and torch.equal(value_out, tr.critic(s))
        args = (s, act[idx], logp[idx], oldv[idx], ret[idx], adv[idx])
        _check_minibatch(f"rows {kind} n={n} train_scaler={int(train)}", tr, psd, vsd, args, stats)
        assert tr._word(8) == 1


def test_a_single_row_minibatch_refuses_to_train_the_scaler():
    pol, val, (obs, act, logp, oldv, ret, adv) = _world()
    tr = _trainer(pol, val)
    blk0, grad0 = tr.state_scaler.clone(), tr.grad.clone()
    from isaac_rover_orbit_amd import _lib
    with pytest.raises(_lib.RoverHipError):
        tr.minibatch(obs, act, logp, oldv, ret, adv, torch.tensor([5], device=DEV), train_scaler=True)
    assert torch.equal(tr.state_scaler, blk0) and torch.equal(tr.grad, grad0) and tr._word(8) == 0


# ------------------------------------------------------------------------------------- 5. stale and oversized workspace
def _run_small(tr, world, n, seed):
    pol, val, (obs, act, logp, oldv, ret, adv) = world
    idx = torch.randperm(8192, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))[:n].contiguous()
    stats = torch.full((4,), -7.0, device=DEV)
    mean_out, value_out = torch.empty(n, 8, device=DEV), torch.empty(n, 1, device=DEV)
    tr.minibatch(obs, act, logp, oldv, ret, adv, idx, stats=stats, mean_out=mean_out, value_out=value_out)
    return tr.grad.clone(), stats, mean_out, value_out


def _poison(tr):
    tr.ws.view(torch.float32).fill_(float("nan"))


@pytest.mark.parametrize("large,small", [(4097, 17), (1000, 1), (513, 64)])
def test_a_small_minibatch_after_a_large_one_reads_only_what_it_wrote(large, small):
    world = _world()
    pol, val = world[0], world[1]
    fresh = _run_small(_trainer(pol, val, kl_early_stop=0.0), world, small, 31)
    tr = _trainer(pol, val, kl_early_stop=0.0)                        # the large call must not stop the epoch
    _run_small(tr, world, large, 30)
    size = tr.ws.numel()
    stale = _run_small(tr, world, small, 31)
    assert tr.ws.numel() == size and tr._word(7) == 0 and tr._word(8) == 2   # the workspace only grows; both calls ran
    for a, b in zip(stale, fresh):
        assert torch.equal(a, b)


@pytest.mark.parametrize("n", [1, 17, 300])
def test_a_nan_filled_oversized_workspace_changes_nothing(n):
    world = _world()
    pol, val = world[0], world[1]
    clean = _trainer(pol, val, kl_early_stop=0.0)
    fresh = _run_small(clean, world, n, 32)
    tr = _trainer(pol, val, kl_early_stop=0.0)
    tr._ensure_ws(4097)
    _poison(tr)
    got = _run_small(tr, world, n, 32)
    for a, b in zip(got, fresh):
        assert torch.equal(a, b) and not bool(torch.isnan(a).any())
    _poison(tr)
    tr.apply()
    clean.apply()
    for name in ("params", "grad", "adam_m", "adam_v", "state", "rep_p", "rep_v"):
        a, b = getattr(tr, name), getattr(clean, name)
        assert torch.equal(a, b) and not bool(torch.isnan(a).any()), name
    moved = not torch.equal(tr.params, _trainer(pol, val).params)
    assert tr.steps == 1 and moved == bool(fresh[0].any())             # a lone row may sit outside both clips: no gradient


# ------------------------------------------------------------------------------------- 6. the scaler entry through the C ABI
class _Scaler:
    """rover_lift_ppo_standardize at any width, with its own block and workspace."""

    def __init__(self, width, **hp):
        from isaac_rover_orbit_amd import _lib
        from isaac_rover_orbit_amd import lift_ppo as LP
        self.lib, self.hp, self.w = _lib.load(), LP.default_hparams(), width
        for k, v in hp.items():
            setattr(self.hp, k, v)
        self.blk = torch.zeros(2 * width + 1, dtype=torch.float64, device=DEV)
        self.blk[width:] = 1.0
        self.ws_bytes = int(self.lib.rover_lift_ppo_workspace_bytes(1))
        self.ws = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=DEV)

    def call(self, x, train=0, inverse=0, out=None, width=None, rows=None, ws="own", ws_bytes=None):
        out = torch.empty_like(x) if out is None else out
        wsp = self.ws.data_ptr() if ws == "own" else ws
        rc = self.lib.rover_lift_ppo_standardize(C.byref(self.hp), self.blk.data_ptr(), self.w if width is None else width, x.data_ptr(),
                                                 x.shape[0] if rows is None else rows, train, inverse, out.data_ptr(), wsp,
                                                 self.ws_bytes if ws_bytes is None else ws_bytes,
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
        return rc, out

    def mean_var(self):
        return self.blk[:self.w].float(), self.blk[self.w:2 * self.w].float()

    def expect(self, x, inverse=False, eps=None, clip=None):
        """The torch expression of test_standardize_bit_identical_and_statistics_match_float64 on this block."""
        eps = float(self.hp.scaler_eps) if eps is None else eps
        clip = float(self.hp.scaler_clip) if clip is None else clip
        mean, var = self.mean_var()
        if inverse:
            return torch.sqrt(var) * torch.clamp(x, min=-clip, max=clip) + mean
        return torch.clamp((x - mean) / (torch.sqrt(var) + eps), min=-clip, max=clip)


def _same_with_nan(a, b):
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


@pytest.mark.parametrize("width", [1, 2, 36, 63, 64])
def test_scaler_entry_at_every_width_and_row_edge(width):
    g = torch.Generator(device=DEV).manual_seed(40 + width)
    col = torch.linspace(0.5, 3.0, width, device=DEV)
    for rows in (2, 255, 256, 257, 1000):
        sc, ali, ns = _Scaler(width), _Scaler(width), NumpyScaler(width)
        for r0, scale, off in ((300, 4.0, 1.5), (77, 0.3, -2.0)):         # two prior updates of different scale and offset
            x = (torch.randn(r0, width, device=DEV, generator=g) * scale * col + off).contiguous()
            assert sc.call(x, train=1)[0] == 0 and ali.call(x, train=1)[0] == 0
            ns.train(x.double().cpu().numpy())
        x = (torch.randn(rows, width, device=DEV, generator=g) * 2.0 * col + 0.5).contiguous()
        x[0, 0], x[1, width - 1] = 1e4, -1e4                              # outside the clamp
        rc, out = sc.call(x, train=1)
        assert rc == 0
        ns.train(x.double().cpu().numpy())
        blk = sc.blk.cpu().numpy()
        np.testing.assert_allclose(blk[:width], ns.mean, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(blk[width:2 * width], ns.var, rtol=1e-12, atol=1e-12)
        assert blk[2 * width] == ns.count == 1 + 300 + 77 + rows
        expect = sc.expect(x)
        assert torch.equal(out, expect) and out.max().item() == 5.0 and out.min().item() == -5.0
        xa = x.clone()
        rc, oa = ali.call(xa, train=1, out=xa)                            # out aliases x
        assert rc == 0 and oa.data_ptr() == xa.data_ptr()
        assert torch.equal(ali.blk, sc.blk) and torch.equal(xa, expect)
        y = (torch.randn(rows, width, device=DEV, generator=g) * 4).contiguous()
        inv = sc.expect(y, inverse=True)
        assert torch.equal(sc.call(y, inverse=1)[1], inv)
        ya = y.clone()
        assert ali.call(ya, inverse=1, out=ya)[0] == 0 and torch.equal(ya, inv)
        assert torch.equal(ali.blk, sc.blk)                               # neither forward nor inverse trains


@pytest.mark.parametrize("width", [2, 36, 64])
def test_scaler_entry_reads_its_eps_and_clip(width):
    g = torch.Generator(device=DEV).manual_seed(50 + width)
    sc, df = _Scaler(width, scaler_eps=1e-3, scaler_clip=2.5), _Scaler(width)
    x0 = (torch.randn(400, width, device=DEV, generator=g) * 0.01 + 1.0).contiguous()   # a small variance: eps counts
    assert sc.call(x0, train=1)[0] == 0 and df.call(x0, train=1)[0] == 0
    assert torch.equal(sc.blk, df.blk)                                    # the statistics do not read eps or clip
    x = (torch.randn(500, width, device=DEV, generator=g) * 0.15 + 1.0).contiguous()
    for inverse in (0, 1):
        xin = (x * 100 - 97).contiguous() if inverse else x
        out = sc.call(xin, inverse=inverse)[1]
        moved, default = sc.expect(xin, bool(inverse)), sc.expect(xin, bool(inverse), eps=1e-8, clip=5.0)
        assert torch.equal(out, moved)
        assert not torch.equal(moved, default)                            # the moved-value inequality: the inputs tell them apart
        assert torch.equal(df.call(xin, inverse=inverse)[1], default)
    fwd = sc.expect(x)
    inner = fwd.abs() < 2.5
    assert bool(inner.any()) and bool((~inner).any())
    assert not torch.equal(fwd[inner], sc.expect(x, eps=1e-8)[inner])     # eps alone is seen on the unclamped entries
    assert fwd.abs().max().item() == 2.5                                  # and clip on the clamped ones


@pytest.mark.parametrize("width", [1, 36, 64])
def test_scaler_entry_with_non_finite_inputs_and_zero_variance(width):
    """clamp propagates NaN as torch.clamp does; +-inf clamp to +-clip; a zero-variance column (a checkpoint can hold one)
    gives +-clip, or 0 / eps = 0 where x equals the mean, and the mean on the way back."""
    g = torch.Generator(device=DEV).manual_seed(60 + width)
    sc = _Scaler(width)
    assert sc.call((torch.randn(300, width, device=DEV, generator=g) * 3 + 1).contiguous(), train=1)[0] == 0
    x = (torch.randn(70, width, device=DEV, generator=g) * 3).contiguous()
    flat = x.view(-1)
    flat[0::7], flat[3::11], flat[5::13] = float("nan"), float("inf"), float("-inf")
    for inverse in (0, 1):
        out, expect = sc.call(x, inverse=inverse)[1], sc.expect(x, bool(inverse))
        assert _same_with_nan(out, expect)
        assert torch.equal(torch.isnan(out), torch.isnan(x)) and bool(torch.isnan(out).any())
        assert not bool(torch.isinf(out).any())
    blk0 = sc.blk.clone()
    zero = list(range(0, width, 3))
    sc.blk[width + torch.tensor(zero, device=DEV)] = 0.0                  # var[c] = 0
    blk1 = sc.blk.clone()
    y = (torch.randn(64, width, device=DEV, generator=g) * 3 + 1).contiguous()
    y[::2, zero] = sc.mean_var()[0][zero]                                 # rows that sit exactly on the mean
    for inverse in (0, 1):
        out, expect = sc.call(y, inverse=inverse)[1], sc.expect(y, bool(inverse))
        assert torch.equal(out, expect) and not bool(torch.isnan(out).any())
        if inverse:
            assert torch.equal(out[:, zero], sc.mean_var()[0][zero].expand(64, -1))
        else:
            assert torch.all(out[::2, zero] == 0.0) and torch.all(out[1::2, zero].abs() == 5.0)
    assert torch.equal(sc.blk, blk1) and not torch.equal(blk1, blk0)


def test_scaler_entry_refusals_leave_the_block_alone():
    sc = _Scaler(36)
    g = torch.Generator(device=DEV).manual_seed(70)
    x = torch.randn(100, 65, device=DEV, generator=g).contiguous()
    assert sc.call(x[:, :36].contiguous(), train=1)[0] == 0
    big = torch.zeros(131, dtype=torch.float64, device=DEV)               # room for any width the entry might believe
    big[:73] = sc.blk
    sc.blk = big
    blk0 = big.clone()
    refusals = [dict(width=0), dict(width=65), dict(rows=1, train=1), dict(train=1, inverse=1), dict(rows=0), dict(rows=0, train=1),
                dict(train=1, ws=None), dict(train=1, ws_bytes=sc.ws_bytes - 4), dict(train=1, ws_bytes=0)]
    for kw in refusals:
        assert sc.call(x, **kw)[0] == INVALID, kw
        torch.cuda.synchronize()
        assert torch.equal(sc.blk, blk0), kw
    assert sc.lib.rover_lift_ppo_scaler_doubles(0) == sc.lib.rover_lift_ppo_scaler_doubles(65) == 0
    assert sc.lib.rover_lift_ppo_scaler_doubles(64) == 129 and sc.lib.rover_lift_ppo_scaler_doubles(2) == 5
    assert sc.call(x[:, :36].contiguous(), ws=None, ws_bytes=0)[0] == 0   # the workspace is train's alone


# ------------------------------------------------------------------------------------- 7. the KL schedule
def _schedule(tr, kls, recorded, n_minibatches=None, stop=0):
    """One kl_schedule call on hand-written stats rows; returns (kl_out, expected kl in float32, in order)."""
    stats = torch.full((len(kls), 4), 123.0, device=DEV)
    stats[:, 0] = torch.tensor(kls, dtype=torch.float32)
    words = tr.state.view(torch.int32)
    words[8], words[7] = recorded, stop
    kl_out = torch.full((1,), -7.0, device=DEV)
    tr.kl_schedule(stats if n_minibatches is None else stats[:n_minibatches], kl_out)
    cnt = min(recorded, len(kls) if n_minibatches is None else n_minibatches)
    acc = np.float32(0.0)
    for k in kls[:cnt]:
        acc = np.float32(acc + np.float32(k))
    return kl_out.item(), (np.float32(acc / np.float32(cnt)) if cnt else None)


KL_MOVED = dict(kl_threshold=0.02, lr_factor=2.0, lr_min=1e-5, lr_max=1e-3)
KL_CASES = [
    # name, hyper-parameters, lr before, KLs, recorded, n_minibatches, branch
    ("grow", {}, 1e-4, [0.001, 0.002, 0.003], 3, None, "up"),
    ("dead-band", {}, 1e-4, [0.006, 0.008, 0.011], 3, None, "same"),
    ("dead-band-low", {}, 1e-4, [0.0045], 1, None, "same"),
    ("dead-band-high", {}, 1e-4, [0.0155], 1, None, "same"),
    ("shrink", {}, 1e-4, [0.02, 0.05], 2, None, "down"),
    ("clamp-at-lr_max", {}, 9e-3, [0.001], 1, None, "max"),
    ("clamp-at-lr_min", {}, 1.2e-6, [0.1], 1, None, "min"),
    ("moved-dead-band", KL_MOVED, 1e-4, [0.03], 1, None, "same"),       # the defaults would shrink
    ("moved-grow", KL_MOVED, 1e-4, [0.007], 1, None, "up"),             # the defaults would hold
    ("moved-shrink", KL_MOVED, 1e-4, [0.05], 1, None, "down"),          # by 2, not 1.5
    ("moved-clamp-at-lr_max", KL_MOVED, 6e-4, [0.001], 1, None, "max"),
    ("moved-clamp-at-lr_min", KL_MOVED, 1.6e-5, [0.3], 1, None, "min"),
    ("more-recorded-than-rows", {}, 1e-4, [0.001, 0.002, 0.9], 3, 2, "up"),     # the mean is over the first 2 rows
    ("fewer-recorded-than-rows", {}, 1e-4, [0.001, 0.002, 0.9], 2, None, "up"),
]


@pytest.mark.parametrize("case", KL_CASES, ids=[c[0] for c in KL_CASES])
def test_kl_schedule_branches(case):
    from isaac_rover_orbit_amd import lift_ppo as LP
    name, hp, lr0, kls, recorded, nmb, branch = case
    pol, val = _nets(9)
    tr = _trainer(pol, val, lr=lr0, **hp)
    h = tr.hp
    assert tr.lr == lr0
    kl, kl_ref = _schedule(tr, kls, recorded, nmb)
    assert np.float32(kl) == kl_ref                                    # the header's order: exact
    want = LP.kl_adaptive(lr0, float(kl_ref), thr=float(h.kl_threshold), factor=float(h.lr_factor), lr_min=float(h.lr_min),
                          lr_max=float(h.lr_max))
    assert tr.lr == pytest.approx(want, rel=1e-12)
    if branch == "same":
        assert tr.lr == lr0                                            # bit-equal
    else:
        assert {"up": want == lr0 * h.lr_factor, "down": want == lr0 / h.lr_factor, "max": want == h.lr_max < lr0 * h.lr_factor,
                "min": want == h.lr_min > lr0 / h.lr_factor}[branch]
    if hp:                                                             # the moved fields are seen
        d = LP.default_hparams()
        assert want != LP.kl_adaptive(lr0, float(kl_ref), thr=float(d.kl_threshold), factor=float(d.lr_factor), lr_min=float(d.lr_min),
                                      lr_max=float(d.lr_max))
    assert (tr._word(7), tr._word(8), tr._word(9), tr.stopped_epochs) == (0, 0, 1, 0)


def test_kl_schedule_with_nothing_recorded_and_its_counters():
    pol, val = _nets(9)
    tr = _trainer(pol, val, lr=3e-4)
    lr_bits = tr.state.view(torch.int64)[0].item()
    kl, _ = _schedule(tr, [0.5, 0.5], 0)
    assert math.isnan(kl) and tr.state.view(torch.int64)[0].item() == lr_bits
    assert (tr._word(7), tr._word(8), tr._word(9), tr.stopped_epochs) == (0, 0, 1, 0)
    kl, _ = _schedule(tr, [0.5, 0.5], 0, stop=1)                       # the counters still advance
    assert math.isnan(kl) and tr.state.view(torch.int64)[0].item() == lr_bits
    assert (tr._word(7), tr._word(8), tr._word(9), tr.stopped_epochs) == (0, 0, 2, 1)
    tr = _trainer(pol, val, lr=3e-4)
    lr = 3e-4
    from isaac_rover_orbit_amd import lift_ppo as LP
    for e, (stop, kls) in enumerate([(0, [0.001, 0.002]), (1, [0.004, 0.03]), (0, [0.01]), (1, [0.02]), (0, [0.0001, 0.0002, 0.0003])]):
        kl, kl_ref = _schedule(tr, kls, len(kls), stop=stop)
        assert np.float32(kl) == kl_ref
        lr = LP.kl_adaptive(lr, float(kl_ref), thr=float(tr.hp.kl_threshold), factor=float(tr.hp.lr_factor),
                            lr_min=float(tr.hp.lr_min), lr_max=float(tr.hp.lr_max))
        assert tr.lr == pytest.approx(lr, rel=1e-12)
        assert tr._word(7) == 0 and tr._word(8) == 0 and tr._word(9) == e + 1
    assert tr._word(9) == 5 and tr.stopped_epochs == 2 and tr.steps == 0
