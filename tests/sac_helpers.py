"""Shared helpers of the SAC tests (test_sac.py, test_gpu_sac_*.py): the example's Gaussian actor, two Q(s, a) critics,
float64 / float32 copies, a fused trainer with both specs, one hyper-parameter dict in rover_sac_hparams' field names for both
paths, seeds picked on the float64 spec so that no clamp or min decision of a run lies within a margin of its discontinuity, and
bit comparisons of two trainers.  td3_helpers' memory fill, error rule and workspace poison are reused."""
import copy

import torch

from ppo_reference import load_example
from td3_helpers import check, copies, err, fill, poison_ws  # noqa: F401  (re-exported for the SAC tests)


def nets(seed=0, device="cpu", bias=None, log_std=None):
    """(policy, critic_1, critic_2): Net(2, True) and two td3.Critic, float32.  ``bias`` sets the actor's output bias (pushes the
    mean towards the action bounds), ``log_std`` the log_std_parameter."""
    from isaac_rover_orbit_amd.td3 import Critic
    ex = load_example()
    torch.manual_seed(seed)
    pol, c1, c2 = ex.Net(2, True), Critic(), Critic()
    with torch.no_grad():
        if bias is not None:
            pol.mlp[6].bias.copy_(torch.tensor(bias))
        if log_std is not None:
            pol.log_std_parameter.copy_(torch.tensor(log_std))
    return pol.to(device), c1.to(device), c2.to(device)


# ---- hyper-parameters: one dict in rover_sac_hparams' field names for both paths
TORCH_NAMES = dict(gamma="discount_factor", polyak="polyak", actor_lr="actor_learning_rate", critic_lr="critic_learning_rate",
                   entropy_lr="entropy_learning_rate", target_entropy="target_entropy", learn_entropy="learn_entropy")
ADAM_NAMES = ("beta1", "beta2", "eps")


def hparams(**hp):
    """(FusedSAC keywords, TorchSAC keywords, Adam settings) of one dict in the C field names.  Every float goes through
    numpy.float32 and back to a Python float first, so both paths hold the number the C struct holds; learn_entropy, the
    struct's one integer, becomes a bool."""
    import numpy as np
    unknown = set(hp) - set(TORCH_NAMES) - set(ADAM_NAMES)
    assert not unknown, unknown
    f = {k: bool(v) if k == "learn_entropy" else float(np.float32(v)) for k, v in hp.items()}
    return f, {TORCH_NAMES[k]: v for k, v in f.items() if k in TORCH_NAMES}, {k: v for k, v in f.items() if k in ADAM_NAMES}


def set_adam(spec, adam):
    """Adam's betas and eps are not TorchSAC hyper-parameters: set them on all three of the spec's optimizers."""
    for opt in (spec.policy_optimizer, spec.critic_optimizer, spec.entropy_optimizer):
        for g in opt.param_groups:
            g["betas"] = (adam.get("beta1", g["betas"][0]), adam.get("beta2", g["betas"][1]))
            g["eps"] = adam.get("eps", g["eps"])


def specs_of(mods, adam=None, **hp):
    """{float64: TorchSAC, float32: TorchSAC} on copies of the modules; ``hp`` in TorchSAC's names, ``adam`` as set_adam takes it."""
    from isaac_rover_orbit_amd.sac import TorchSAC
    out = {dt: TorchSAC(*copies(mods, dt), **hp) for dt in (torch.float64, torch.float32)}
    for sp in out.values():
        set_adam(sp, adam or {})
    return out


def _f32(x):
    import numpy as np
    return None if x is None else float(np.float32(x))


def specs(mods, log_entropy_coefficient=None, **hp):
    """specs_of for ``hp`` in rover_sac_hparams' field names (see hparams): what ``trainers`` puts beside the fused trainer."""
    _, torch_kw, adam = hparams(**hp)
    return specs_of(mods, adam=adam, log_entropy_coefficient=_f32(log_entropy_coefficient), **torch_kw)


def trainers(mods, log_entropy_coefficient=None, n_copies=4, **hp):
    """(FusedSAC, specs) with the same networks and the same hyper-parameters (``hp`` in rover_sac_hparams' field names, see
    hparams).  ``log_entropy_coefficient`` starts log_alpha on both paths at that number's float32."""
    from isaac_rover_orbit_amd.sac import FusedSAC
    fused = FusedSAC(*(m.state_dict() for m in mods), log_entropy_coefficient=_f32(log_entropy_coefficient), n_copies=n_copies,
                     **hparams(**hp)[0])
    return fused, specs(mods, log_entropy_coefficient, **hp)


def sample(mem, idx, dt):
    s, a, r, s2, t = mem.gather(idx)
    return s.to(dt), a.to(dt), r.to(dt), s2.to(dt), t


def grads(module):
    return {k: p.grad.detach().clone() for k, p in module.named_parameters()}


def params(module):
    return {k: p.detach().clone() for k, p in module.named_parameters()}


def draws(n, seed, device="cpu", scale=1.0):
    """eps (n, 4) float32: columns 0:2 for s', columns 2:4 for s."""
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randn(n, 4, device=device, generator=g) * scale


def decision_margin(spec, st, e, qa, qb):
    """The smallest | |x| - 1 | and | qa - qb | over the rows of states ``st`` with the draws ``e`` (n, 2)."""
    from isaac_rover_orbit_amd.sac import LOG_STD_MAX, LOG_STD_MIN
    with torch.no_grad():
        sigma = spec.policy.log_std_parameter.clamp(LOG_STD_MIN, LOG_STD_MAX).exp()
        x = spec.policy(st) + sigma * e.to(spec.dtype)
        u = x.clamp(-1.0, 1.0)
        return min(float((x.abs() - 1.0).abs().min()), float((qa(st, u) - qb(st, u)).abs().min()))


class HiddenMargin:
    """Context manager: ``.value`` is the smallest | pre-activation | of any hidden unit (every Linear but the last) of
    ``modules`` over the forwards run inside it -- the distance of the nearest LeakyReLU' decision from flipping.  Give it the
    networks a step differentiates through: the critics for the critic step, the policy and the critics for the policy step."""

    def __init__(self, *modules):
        self.modules, self.handles, self.value = modules, [], float("inf")

    def _see(self, _module, _inputs, out):
        self.value = min(self.value, float(out.detach().abs().min()))

    def __enter__(self):
        for m in self.modules:
            linears = [x for x in m.modules() if isinstance(x, torch.nn.Linear)]
            self.handles += [x.register_forward_hook(self._see) for x in linears[:-1]]
        return self

    def __exit__(self, *exc):
        for h in self.handles:
            h.remove()
        return False


def update_with_margin(spec, mem, idx, eps):
    """``spec.update(mem, idx, eps)`` in its pieces; returns the smallest | |x| - 1 | and | q1 - q2 | over the rows, each read where
    the update decides it: the target pair on (s', u') before the critic step, the critics on (s, u) after it."""
    s, a, r, s2, t = sample(mem, idx, spec.dtype)
    m = decision_margin(spec, s2, eps[:, 0:2], spec.target_critic_1, spec.target_critic_2)
    spec.critic_step(s, a, r, s2, t, eps[:, 0:2])
    m = min(m, decision_margin(spec, s, eps[:, 2:4], spec.critic_1, spec.critic_2))
    spec.policy_step(s, eps[:, 2:4])
    spec.polyak()
    return m


def clone_modules(mods):
    return [copy.deepcopy(m) for m in mods]


# ---- bit comparisons of two fused trainers (td3_helpers' pair, without TD3's host-side update count)
TRAINER_VECTORS = ("params", "target", "grad", "adam_m", "adam_v", "state", "rep_a")


def clone_trainer(src, dst):
    """Copies src's device vectors into dst (a FusedSAC of the same hyper-parameters and replica count)."""
    for name in TRAINER_VECTORS:
        getattr(dst, name).copy_(getattr(src, name))


def assert_same_trainer(a, b, skip_state_words=()):
    """Every device vector of two trainers bit for bit (state words in skip_state_words left out)."""
    for name in TRAINER_VECTORS:
        x, y = getattr(a, name), getattr(b, name)
        if name == "state" and skip_state_words:
            keep = [i for i in range(x.numel()) if i not in skip_state_words]
            x, y = x[keep], y[keep]
        # equal as numbers (a NaN on either side fails) and as bit patterns (-0 is not +0)
        assert torch.equal(x, y) and torch.equal(x.view(torch.int32), y.view(torch.int32)), name
