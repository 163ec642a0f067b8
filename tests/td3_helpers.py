"""Shared helpers of the TD3 tests (test_td3.py, test_gpu_td3_*.py): the example's actor, the Q(s, a) critic, a filled replay
memory, float64 / float32 copies of the networks, the "fused error <= 4x torch fp32 error against float64, plus a floor" check
of trpo_helpers, one hyper-parameter dict for both paths and bit comparisons of two trainers."""
import copy

import torch

from ppo_reference import load_example


def nets(seed=0, device="cpu"):
    """(actor, critic_1, critic_2): Net(2, False) and two td3.Critic, float32."""
    from isaac_rover_orbit_amd.td3 import Critic
    ex = load_example()
    torch.manual_seed(seed)
    pol, c1, c2 = ex.Net(2, False), Critic(), Critic()
    return pol.to(device), c1.to(device), c2.to(device)


def copies(mods, dtype):
    return [copy.deepcopy(m).to(dtype) for m in mods]


def fill(memory, steps, seed=1, term_p=0.1, obs_scale=0.5, identity=True):
    """``steps`` adds in the reference's loop order (states of add t + 1 = next_states of add t).  identity=True passes the
    same tensor on (the example's loop), False copies into a persistent buffer (the reference's states.copy_(next_states))."""
    dev = memory.obs.device
    g = torch.Generator(device=dev).manual_seed(seed)
    N, D, A = memory.num_envs, memory.obs.shape[-1], memory.actions.shape[-1]
    states = torch.randn(N, D, device=dev, generator=g) * obs_scale
    hist = []
    for _ in range(steps):
        actions = torch.rand(N, A, device=dev, generator=g) * 2 - 1
        rewards = torch.randn(N, 1, device=dev, generator=g)
        next_states = torch.randn(N, D, device=dev, generator=g) * obs_scale
        terminated = torch.rand(N, 1, device=dev, generator=g) < term_p
        memory.add(states, actions, rewards, next_states, terminated)
        hist.append((states.clone(), actions, rewards, next_states, terminated))
        if identity:
            states = next_states
        else:
            states = states.clone()
            states.copy_(next_states)
    return hist


def err(a, ref):
    return float((a.double().cpu() - ref.double().cpu()).norm())


def check(fused, ref64, ref32, factor=4.0, floor=1e-5, what=""):
    """fused / ref32: tensors or dicts of tensors; the fused error against float64 within factor x torch fp32's, plus a floor."""
    if isinstance(ref64, dict):
        for k in ref64:
            check(fused[k], ref64[k], ref32[k], factor, floor, f"{what}{k}")
        return
    e_f, e_t = err(fused, ref64), err(ref32, ref64)
    assert e_f <= factor * e_t + floor * float(ref64.double().norm()) + 1e-30, (what, e_f, e_t, float(ref64.norm()))


# ---- hyper-parameters: one dict in rover_td3_hparams' field names for both paths
TORCH_NAMES = dict(gamma="discount_factor", polyak="polyak", actor_lr="actor_learning_rate", critic_lr="critic_learning_rate",
                   noise_clip="smooth_regularization_clip", act_min="clip_actions_min", act_max="clip_actions_max")
ADAM_NAMES = ("beta1", "beta2", "eps")


def hparams(**hp):
    """(FusedTD3 keywords, TorchTD3 keywords, Adam settings) of one dict in the C field names.  Every value goes through
    numpy.float32 and back to a Python float first, so both paths hold the number the C struct holds."""
    import numpy as np
    unknown = set(hp) - set(TORCH_NAMES) - set(ADAM_NAMES)
    assert not unknown, unknown
    f = {k: float(np.float32(v)) for k, v in hp.items()}
    return f, {TORCH_NAMES[k]: v for k, v in f.items() if k in TORCH_NAMES}, {k: v for k, v in f.items() if k in ADAM_NAMES}


def set_adam(spec, adam):
    """Adam's betas and eps are not TorchTD3 hyper-parameters: set them on both of the spec's optimizers."""
    for opt in (spec.policy_optimizer, spec.critic_optimizer):
        for g in opt.param_groups:
            g["betas"] = (adam.get("beta1", g["betas"][0]), adam.get("beta2", g["betas"][1]))
            g["eps"] = adam.get("eps", g["eps"])


def trainers(mods, policy_delay=2, **hp):
    """(FusedTD3, {float64: TorchTD3, float32: TorchTD3}) from (actor, critic_1, critic_2) with the same hyper-parameters."""
    from isaac_rover_orbit_amd.td3 import FusedTD3, TorchTD3
    fused_kw, torch_kw, adam = hparams(**hp)
    fused = FusedTD3(*(m.state_dict() for m in mods), policy_delay=policy_delay, **fused_kw)
    specs = {}
    for dt in (torch.float64, torch.float32):
        specs[dt] = TorchTD3(*copies(mods, dt), policy_delay=policy_delay, **torch_kw)
        set_adam(specs[dt], adam)
    return fused, specs


def poison_ws(fused, rows):
    """Grows the trainer's workspace to ``rows`` rows and fills it with 0xFF bytes: every float in it is a NaN."""
    fused._ensure_ws(rows)
    fused.ws.fill_(0xFF)


TRAINER_VECTORS = ("params", "target", "grad", "adam_m", "adam_v", "state", "rep_a")


def clone_trainer(src, dst):
    """Copies src's device vectors and step count into dst (a FusedTD3 of the same hyper-parameters)."""
    for name in TRAINER_VECTORS:
        getattr(dst, name).copy_(getattr(src, name))
    dst.critic_updates = src.critic_updates


def assert_same_trainer(a, b, skip_state_words=()):
    """Every device vector of two trainers bit for bit (state words in skip_state_words left out)."""
    for name in TRAINER_VECTORS:
        x, y = getattr(a, name), getattr(b, name)
        if name == "state" and skip_state_words:
            keep = [i for i in range(x.numel()) if i not in skip_state_words]
            x, y = x[keep], y[keep]
        # equal as numbers (a NaN on either side fails) and as bit patterns (-0 is not +0)
        assert torch.equal(x, y) and torch.equal(x.view(torch.int32), y.view(torch.int32)), name
    assert a.critic_updates == b.critic_updates


# ---- the collector's edge cases (test_td3_collect.py on the spec, test_gpu_td3_collect_edges.py on the kernels)
INF = float("inf")
# exploration hyper-parameters under explore = 1: name -> (noise_std, noise_scale, low, high).  1e30 * |eps| * 1e30 overflows fp32
# for every |eps| > 3.5e-22, i.e. for every draw: the second product is +/-inf and the clamp returns a bound.
EXPLORE_CASES = {"low_equals_high": (0.3, 0.7, 0.25, 0.25),
                 "unbounded": (0.3, 0.7, -INF, INF),
                 "zero_scale": (0.3, 0.0, -1.0, 1.0),
                 "negative_scale": (0.3, -0.7, -1.0, 1.0),
                 "overflowing_noise": (1e30, 1e30, -0.5, 0.75)}

# the top of the draws' ranges: the last of 33 ids is 2**31 - 2, every key bit set, counters around 2**32 and at 2**64 - 1
TOP_OFFSET, TOP_SEED, TOP_COUNTERS = 2 ** 31 - 34, 2 ** 64 - 1, (2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1)

# index draws: the top of mem_rows with batches that end one and three positions into a Philox block, and one below / above 1024
INDEX_MEM_ROWS, INDEX_BATCHES = (2 ** 31, 2 ** 32 - 1, 2 ** 32), (3, 5, 1023, 1025)


def check_explore_case(name, act, mean, eps):
    """``act`` bit for bit against td3.explore in fp32 torch on ``mean`` and ``eps``, and what the case is there to show."""
    from isaac_rover_orbit_amd.td3 import explore
    std, scale, low, high = EXPLORE_CASES[name]
    want = explore(mean, std * eps, scale, low, high)
    assert same_bits_nan_aware(act, want), name
    if name == "low_equals_high":
        assert bool((act == low).all())
    elif name == "unbounded":
        assert same_bits_nan_aware(act, mean + (std * eps) * scale) and not same_bits_nan_aware(act, (mean + (std * eps) * scale).clamp(-1, 1))
    elif name == "zero_scale":
        assert same_bits_nan_aware(act, (mean + (std * eps) * 0.0).clamp(low, high))
    elif name == "negative_scale":
        plus = explore(mean, std * eps, -scale, low, high)
        assert not same_bits_nan_aware(act, plus)
    elif name == "overflowing_noise":
        assert bool(((act == low) | (act == high)).all()) and bool((act == low).any()) and bool((act == high).any())
        assert bool(torch.isinf((std * eps) * scale).all())


def same_bits_nan_aware(a, b):
    """NaN at the same places (whatever its payload) and every other element equal on the bits."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    x, y = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return bool(torch.equal(na, nb)) and bool(torch.equal(x[~na], y[~nb]))


def eps_float64_by_hand(seed, ids, counter, width, tag):
    """The exploration draws in Python integers and math.* (Random123's Philox4x32-10, the uniforms and Box-Muller of
    include/rover_td3_collect.h), independent of the numpy text of rollout.standard_normals."""
    import math
    F = 0xFFFFFFFF
    out = []
    for g in ids:
        row = []
        for p in range((width + 1) // 2):
            c, k = [int(g) & F, counter & F, (counter >> 32) & F, tag | p], [seed & F, (seed >> 32) & F]
            for _ in range(10):
                p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
                c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & F, (p0 >> 32) ^ c[3] ^ k[1], p0 & F]
                k = [(k[0] + 0x9E3779B9) & F, (k[1] + 0xBB67AE85) & F]
            u1, u2 = ((c[0] >> 9) + 0.5) * 2.0 ** -23, ((c[1] >> 9) + 0.5) * 2.0 ** -23
            rho = math.sqrt(-2.0 * math.log(u1))
            row += [rho * math.cos(2.0 * math.pi * u2), rho * math.sin(2.0 * math.pi * u2)]
        out.append(row[:width])
    return out
