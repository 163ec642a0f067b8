"""Shared helpers of the DAgger edge tests (test_dagger.py, test_gpu_dagger_collect_edges.py, test_gpu_dagger_update_edges.py): thin
ctypes wrappers around the four launching entry points of include/rover_dagger.h next to ``_lib.DaggerHparams``, the mixing draw in
Python integers, the values and places of the rows tests, the float64 scalars of a batch without a step, the float64 / float32
references of one step from the fused trainer's own parameters, and one Adam step in float64 with the bound an fp32 evaluation meets."""
import copy
import ctypes as C
import math

import numpy as np
import torch

FLT_MAX = float(np.finfo(np.float32).max)
RANDOM_TAG = 0x54335200            # include/rover_td3_explore.h: ROVER_TD3_TAG_RANDOM, written out so that the check is its own text


def f32(x):
    return float(np.float32(x))


def bits_of(x):
    return int(np.float32(x).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- C wrappers
def hparams(**kw):
    """``rover_dagger_default_hparams`` with fields moved; ``seed`` sets both key words."""
    from isaac_rover_orbit_amd import dagger
    hp = dagger.default_hparams()
    seed = kw.pop("seed", None)
    if seed is not None:
        hp.seed_lo, hp.seed_hi = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for k, v in kw.items():
        assert hasattr(hp, k), k
        setattr(hp, k, v)
    return hp


def _ptr(t):
    return None if t is None else t.data_ptr()


def rows(hp, depth, env_raw, n, rows_out, teacher_rows_out=None):
    """One ``rover_dagger_rows`` launch on the current stream; tensors of any shape, only their pointers are passed."""
    from isaac_rover_orbit_amd._fused import launch
    launch("rover_dagger_rows", depth.device, C.byref(hp), depth.data_ptr(), env_raw.data_ptr(), int(n), rows_out.data_ptr(),
           _ptr(teacher_rows_out))


def record(hp, depth, env_raw, n, ring_slot, teacher_rows_out=None, counter=0, *, rew=None, terminated=None, rew_out=None, term_out=None,
           ring_pos_entry=None, ring_pos_value=0, idx_out=None, batch=None, mem_rows=0):
    """One ``rover_dagger_record`` launch; ``batch`` defaults to the size of ``idx_out`` (0 without it)."""
    from isaac_rover_orbit_amd._fused import launch
    if batch is None:
        batch = 0 if idx_out is None else int(idx_out.numel())
    launch("rover_dagger_record", depth.device, C.byref(hp), depth.data_ptr(), env_raw.data_ptr(), int(n), ring_slot.data_ptr(),
           _ptr(teacher_rows_out), _ptr(rew), _ptr(terminated), _ptr(rew_out), _ptr(term_out), _ptr(ring_pos_entry), int(ring_pos_value),
           _ptr(idx_out), int(batch), int(mem_rows), C.c_uint64(int(counter)))


def act(teacher, student, hp, counter, beta, teacher_rows, student_rows, n, label_out, env_act_out, student_out=None, source_out=None):
    """One ``rover_dagger_act`` call (two launches) with two ``RoverNet`` and the rows given by pointer."""
    from isaac_rover_orbit_amd._fused import launch
    launch("rover_dagger_act", student_rows.device, C.byref(teacher.desc), teacher.packed.data_ptr(), teacher.n_copies, C.byref(student.desc),
           student.packed.data_ptr(), student.n_copies, C.byref(hp), C.c_uint64(int(counter)), C.c_float(beta), teacher_rows.data_ptr(),
           student_rows.data_ptr(), int(n), label_out.data_ptr(), env_act_out.data_ptr(), _ptr(student_out), _ptr(source_out))


def update_args(fused, mem, idx, dz_out=None, replicas=True):
    """The argument list of ``rover_dagger_update`` for a FusedDAgger as ``FusedDAgger.update`` forms it, without the stream; a
    dict, so that a refusal test can move one argument at a time."""
    n = fused._sample(mem, idx)
    return dict(student=C.byref(fused.desc_a), hp=C.byref(fused.hp), params=fused.params.data_ptr(), grad=fused.grad.data_ptr(),
                adam_m=fused.adam_m.data_ptr(), adam_v=fused.adam_v.data_ptr(), obs=mem.obs.data_ptr(), slots=mem.slots,
                num_envs=mem.num_envs, ring_pos=mem.ring_pos.data_ptr(), labels=mem.actions.data_ptr(), idx=idx.data_ptr(), n=n,
                valid_rows=len(mem), ws=fused.ws.data_ptr(), ws_bytes=fused.ws.numel(), state=fused.state.data_ptr(),
                replicas=fused.rep_a.data_ptr() if replicas else None, n_copies=fused.n_copies, dz_out=_ptr(dz_out))


UPDATE_ORDER = ("student", "hp", "params", "grad", "adam_m", "adam_v", "obs", "slots", "num_envs", "ring_pos", "labels", "idx", "n",
                "valid_rows", "ws", "ws_bytes", "state", "replicas", "n_copies", "dz_out")


def update_call(fused, args):
    """``rover_dagger_update`` on the current stream; returns the code."""
    from isaac_rover_orbit_amd import _lib
    from isaac_rover_orbit_amd._fused import stream
    with torch.cuda.device(fused.device):
        return _lib.load().rover_dagger_update(*(args[k] for k in UPDATE_ORDER), stream(fused.device))


def update(fused, mem, idx, dz_out=None, replicas=True):
    from isaac_rover_orbit_amd import _lib
    _lib.check(update_call(fused, update_args(fused, mem, idx, dz_out, replicas)), "rover_dagger_update")


# ---------------------------------------------------------------------------------------------------------------- the draw
def mix_uniforms_by_hand(seed, ids, counter):
    """The mixing draws in Python integers: the Philox4x32-10 rounds of td3_helpers.eps_float64_by_hand on the counter
    (g, counter_lo, counter_hi, RANDOM_TAG) and u = ((w0 >> 9) + 0.5) * 2**-23, independent of the numpy text of td3_explore."""
    F = 0xFFFFFFFF
    out = []
    for g in ids:
        c, k = [int(g) & F, counter & F, (counter >> 32) & F, RANDOM_TAG], [seed & F, (seed >> 32) & F]
        for _ in range(10):
            p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
            c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & F, (p0 >> 32) ^ c[3] ^ k[1], p0 & F]
            k = [(k[0] + 0x9E3779B9) & F, (k[1] + 0xBB67AE85) & F]
        out.append(((c[0] >> 9) + 0.5) * 2.0 ** -23)
    return out


# ---------------------------------------------------------------------------------------------------------------- the rows
ENV_PLACES = (0, 1, 2, 3)                                   # the proprioceptive columns of every row
PIXEL_PLACES = (0, 1, 2, 3, 957, 958, 959, 960)             # the pixels of the pieces that straddle a row's head, and the row's last


def pixel_values(special_bits, depth_clip):
    """Bit patterns a pixel takes: the special values (-0.0 is one of them), the clip itself and the float after it."""
    assert 0x80000000 in special_bits
    with np.errstate(over="ignore"):                        # the float after FLT_MAX is +inf
        after = np.nextafter(np.float32(depth_clip), np.float32(np.inf))
    return list(special_bits) + [bits_of(depth_clip), bits_of(after)]


def _signed(b):
    return b - (1 << 32) if b >= 1 << 31 else b


def plant(depth, env, n, special_bits, depth_clip, rot):
    """Plants the special values into flat views ``depth`` (n * 961) and ``env`` (n * 965) in place: place j of a row takes value
    (j + rot) mod the number of values, and so do the last two floats of the env buffer."""
    pv = pixel_values(special_bits, depth_clip)
    d, e = depth.view(torch.int32), env.view(torch.int32)
    for r in range(n):
        for j, c in enumerate(ENV_PLACES):
            e[r * 965 + c] = _signed(special_bits[(j + rot + r) % len(special_bits)])
        for j, p in enumerate(PIXEL_PLACES):
            d[r * 961 + p] = _signed(pv[(j + rot + r) % len(pv)])
    for j, g in enumerate((n * 965 - 2, n * 965 - 1)):
        e[g] = _signed(special_bits[(len(ENV_PLACES) + j + rot) % len(special_bits)])


# ---------------------------------------------------------------------------------------------------------------- the update
def reference_scalars(spec, mem, idx):
    """loss, grad_norm and the rows' d^2 (n,) of a TorchDAgger on the batch, from a copy of its student: no step is taken."""
    m = copy.deepcopy(spec.student)
    s, a, *_ = mem.gather(idx)
    dt = next(m.parameters()).dtype
    out = m(s.to(dt))
    d2 = ((out - a.to(dt)) ** 2).sum(1)
    loss = d2.sum() / (2 * idx.numel())
    loss.backward()
    sq = sum(float((p.grad.double() ** 2).sum()) for p in m.parameters() if p.grad is not None)
    return {"loss": float(loss.detach()), "grad_norm": math.sqrt(sq), "d2": d2.detach()}


def strict_update(mem, fused, specs, idx, steps_before=0, scalars=("loss", "grad_norm")):
    """test_gpu_dagger.check_update, with test_gpu_td3_hparams_edges.check_stats' condition on ``scalars``: the float64 value
    exceeds 1e-3, so check_update's relative bound of 1e-3 decides and its absolute 1e-6 does not."""
    from test_gpu_dagger import check_update
    want = reference_scalars(specs[torch.float64], mem, idx)
    for k in scalars:
        assert want[k] > 1e-3, (k, want[k])
    st, dz = check_update(mem, fused, specs, idx, steps_before)
    return st, dz, want


def reference_at(fused, specs, mem, idx):
    """{dtype: (loss, grad_norm, gradients by name)} of the float64 and float32 torch students holding the FUSED trainer's current
    parameters: the references of one step from where the fused trainer stands, whatever its trajectory was."""
    out = {}
    sd = fused.unvector(fused.params)["policy"]
    s, a, *_ = mem.gather(idx)
    for dt, spec in specs.items():
        m = copy.deepcopy(spec.student)
        m.load_state_dict({k: v.to(dt).to(s.device) for k, v in sd.items()}, strict=False)
        loss = ((m(s.to(dt)) - a.to(dt)) ** 2).sum() / (2 * idx.numel())
        loss.backward()
        g = {k: p.grad.detach() for k, p in m.named_parameters() if p.grad is not None}
        out[dt] = (float(loss.detach()), math.sqrt(sum(float((v.double() ** 2).sum()) for v in g.values())), g)
    return out


ULP = 2.0 ** -24


def adam_step_float64(p, g, m, v, t, lr, beta1, beta2, eps):
    """One Adam step in float64 on flat float64 vectors (torch's single-tensor order, include/rover_dagger.h) and, per element, how far
    an fp32 evaluation of the same step may lie from it.  Counted in roundings of 2**-24 (ULP):
      m' = beta1 m + (1 - beta1) g        three roundings of terms no larger than |m| + |g| (1 - beta is exact in fp32 for beta >= 0.5)
      v' = beta2 v + (1 - beta2) g^2      four roundings of positive terms: 4 ULP of v' itself
      u  = s m' / (sqrt(v') / b + eps)    s and b each within 2.5e-7 = 4.2 ULP of their float64 values (the bound their own test holds
                                          them to), sqrt(v') 2 + 1, the quotient by b 1, the sum 1, the quotient 1, the product 1:
                                          16 ULP of |u|, plus m's own error through s / denominator
      p' = p - u                          one rounding of max(|p|, |p'|)
    and a floor of 1e-37 where a term is denormal."""
    s, b = lr / (1.0 - beta1 ** t), math.sqrt(1.0 - beta2 ** t)
    m2 = beta1 * m + (1.0 - beta1) * g
    v2 = beta2 * v + (1.0 - beta2) * g * g
    den = v2.sqrt() / b + eps
    u = s * m2 / den
    p2 = p - u
    tol_m = 4 * ULP * (m.abs() + g.abs()) + 1e-37
    tol_v = 4 * ULP * v2 + 1e-37
    tol_p = ULP * torch.maximum(p.abs(), p2.abs()) + 16 * ULP * u.abs() + tol_m * s / den + 1e-37
    return (p2, tol_p), (m2, tol_m), (v2, tol_v)
