"""The Python host plumbing that the fused trainers and collectors share: plain functions first, then the trainers' base
classes, which hold only the state every trainer has.

What is particular to a trainer stays in its module: which networks it packs, the layout of its parameter vector, its state block
and its launches.  The torch specifications (``Torch*``) share nothing with this module on purpose: they are the independent side
of every comparison in the suite.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Mapping

import numpy as np
import torch

from . import _lib

_MASK = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------------------- launches
def stream(device) -> C.c_void_p:
    """The current torch stream of ``device`` as the ``hipStream_t`` argument of a library call."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    """``t.data_ptr()``, or NULL for ``None``."""
    return None if t is None else t.data_ptr()


def launch(fn: str, device, *args) -> None:
    """One call of the library's ``fn`` on the current stream of ``device``, the stream as its last argument."""
    s = stream(device)
    with torch.cuda.device(device):
        _lib.check(getattr(_lib.load(), fn)(*args, s), fn)


def f32_cuda(name: str, t, device, on: str = "the actor's device") -> None:
    if t is not None and (not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.device != device):
        raise ValueError(f"{name} must be a contiguous float32 cuda tensor on {on}")


def holds(name: str, t, shape) -> None:
    """Refuses a tensor (``None`` passes) that does not hold ``prod(shape)`` values; ``shape`` an int or a tuple of ints."""
    if t is not None and t.numel() != (shape if isinstance(shape, int) else math.prod(shape)):
        raise ValueError(f"{name} must hold {shape} values")


def layout_pitch(shape, stride, contiguous: bool, width: int, rows: int | None = None):
    """The layout half of ``row_pitch``: the pitch of a tensor of this shape, strides and contiguity, or None where it is refused."""
    if len(shape) < 2 or (rows is not None and shape[0] != rows):
        return None
    if len(shape) == 2 and shape[1] == width and stride[1] == 1 and (shape[0] == 1 or stride[0] >= width):
        return stride[0] if shape[0] > 1 else width
    return width if contiguous and math.prod(shape) == shape[0] * width else None


def row_pitch(name: str, t, width: int, rows: int | None = None, device=None) -> int:
    """The row pitch, in floats, of a float32 cuda tensor that holds ``width`` consecutive values per row: 2-D ``(n, width)`` with
    unit column stride and any pitch >= width (one row: any), or contiguous ``(n, ...)``; ``rows`` and ``device`` are checked where
    given.  The one statement of the rule for the observation post-processing, the depth sensor, the elevation map and the lidar."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or (device is not None and t.device != device):
        raise ValueError(f"{name} must be a float32 cuda tensor" + ("" if device is None else f" on {device}"))
    pitch = layout_pitch(tuple(t.shape), t.stride(), t.is_contiguous(), width, rows)
    if pitch is None:
        raise ValueError(f"{name} must hold {width} consecutive values per row" + ("" if rows is None else f", {rows} rows")
                         + ": (n, width) with unit column stride or contiguous (n, ...)")
    return int(pitch)


def check_tensor(t: torch.Tensor, name: str, dtype=torch.float32) -> None:
    if not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} cuda tensor")


def require_gpu(name: str, spec: str | None = None) -> None:
    """``spec``: the clause that names the CPU specification, e.g. ``"TorchRollout is the CPU specification"``."""
    if not torch.cuda.is_available():
        raise _lib.RoverHipError(f"{name} needs a ROCm GPU (no CPU fallback{'' if spec is None else '; ' + spec})")


def seeded(hp, seed: int, env_id_offset: int):
    """The seed / offset part of a collector's hparams struct."""
    hp.seed_lo, hp.seed_hi = seed & _MASK, (seed >> 32) & _MASK
    hp.env_id_offset = env_id_offset
    return hp


# ------------------------------------------------------------------------------------------------ hparams, checkpoints, state
def default_hparams(struct_cls, fn_name: str):
    h = struct_cls()
    _lib.check(getattr(_lib.load(), fn_name)(C.byref(h)), fn_name)
    return h


def set_hparams(hp, overrides: Mapping, convert: Mapping | None = None):
    """``setattr(hp, k, v)`` of each override, refusing names the struct does not have; ``convert[k]`` maps a value first."""
    for k, v in overrides.items():
        if not hasattr(hp, k):
            raise TypeError(f"unknown hyper-parameter {k!r}")
        setattr(hp, k, convert[k](v) if convert and k in convert else v)
    return hp


def load_checkpoint(ck):
    """A checkpoint given as a path or as the loaded dict."""
    if isinstance(ck, str):
        ck = torch.load(ck, map_location="cpu", weights_only=False)
    return ck


def read_state(struct_cls, tensor: torch.Tensor) -> dict:
    """The fields of a device struct (one host synchronisation), without its ``reserved*`` padding."""
    st = struct_cls.from_buffer_copy(tensor.cpu().numpy().tobytes())
    return {f: getattr(st, f) for f, *_ in struct_cls._fields_ if not f.startswith("reserved")}


# -------------------------------------------------------------------------------------------------------------- pack / unpack
def host_layers(sd: Mapping[str, torch.Tensor], key_patterns):
    """(weights, biases, layers found per pattern): for each pattern in turn, ``pattern.format(2 * i, "weight" / "bias")`` for
    i = 0, 1, ... while present, as contiguous float32 host arrays."""
    ws, bs, counts = [], [], []
    for pat in key_patterns:
        i = 0
        while pat.format(2 * i, "weight") in sd:
            ws.append(sd[pat.format(2 * i, "weight")]); bs.append(sd[pat.format(2 * i, "bias")])
            i += 1
        counts.append(i)
    ws = [np.ascontiguousarray(torch.as_tensor(w).detach().cpu().numpy(), dtype=np.float32) for w in ws]
    bs = [np.ascontiguousarray(torch.as_tensor(b).detach().cpu().numpy(), dtype=np.float32) for b in bs]
    return ws, bs, counts


def _pointers(arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def pack_layers(desc: "_lib.PolicyDesc", ws, bs, entry: str = "rover_policy_pack") -> np.ndarray:
    """The packed host array of the layers of ``desc``."""
    lib = _lib.load()
    packed = np.empty(int(lib.rover_policy_packed_floats(C.byref(desc))), dtype=np.float32)
    _lib.check(getattr(lib, entry)(C.byref(desc), _pointers(ws), _pointers(bs), packed.ctypes.data), entry)
    return packed


def unpack_layers(desc: "_lib.PolicyDesc", packed):
    """Packed buffer (one replica) -> (weights, biases) as float32 CPU tensors (``rover_policy_unpack``)."""
    packed = np.ascontiguousarray(torch.as_tensor(packed).detach().cpu().numpy(), dtype=np.float32)
    nl = desc.n_enc + desc.n_mlp
    ws = [np.empty((desc.layers[i].N, desc.layers[i].K), np.float32) for i in range(nl)]
    bs = [np.empty(desc.layers[i].N, np.float32) for i in range(nl)]
    _lib.check(_lib.load().rover_policy_unpack(C.byref(desc), packed.ctypes.data, _pointers(ws), _pointers(bs)), "rover_policy_unpack")
    return [torch.from_numpy(w) for w in ws], [torch.from_numpy(b) for b in bs]


# ------------------------------------------------------------------------------------------------------------------- trainers
class FusedTrainer:
    """What the five fused trainers hold alike: the library, the device, the hparams struct, the flat vectors ``params`` / ``grad`` /
    ``adam_m`` / ``adam_v``, the workspace and the reading of the device state struct.  A subclass names its entries below."""

    _STATE = None            # the ctypes mirror of the device state struct that ``stats`` reads
    _WORKSPACE = ""          # the rover_*_workspace_bytes(rows) entry
    _PARAM_FLOATS = ""       # the rover_*_param_floats(desc, desc) entry
    _RUNS = ""               # what the trainer runs, for the refusal of any other architecture

    def __init__(self, default, hparams: Mapping, device, n_copies: int, convert: Mapping | None = None):
        require_gpu(type(self).__name__)
        self._lib = _lib.load()
        self.device = torch.device(device)
        self.hp = set_hparams(default(), hparams, convert)
        self.n_copies = int(n_copies)
        self._ws_bytes = getattr(self._lib, self._WORKSPACE)

    def _param_floats(self, desc_1, desc_2) -> int:
        P = int(getattr(self._lib, self._PARAM_FLOATS)(C.byref(desc_1), C.byref(desc_2)))
        if P == 0:
            raise _lib.RoverHipError(f"{type(self).__name__} runs {self._RUNS}")
        return P

    def _alloc(self, flat: np.ndarray) -> None:
        self.params = torch.from_numpy(flat).to(self.device)
        self.grad = torch.zeros_like(self.params)
        self.adam_m = torch.zeros_like(self.params)
        self.adam_v = torch.zeros_like(self.params)
        self.ws = torch.empty(0, dtype=torch.uint8, device=self.device)

    def _replica(self, desc, block: torch.Tensor):
        """(the ``n_copies`` replicas of a parameter block that the inference kernels read, the ``RoverNet`` on them)."""
        from .policy import RoverNet      # policy.py takes ``stream`` from this module
        rep = block.repeat(self.n_copies)
        return rep, RoverNet.from_packed(desc, rep, self.n_copies)

    @classmethod
    def from_checkpoint(cls, ck, **kw):
        """A checkpoint (a path or the loaded dict) with the keys of ``_checkpoint_args``."""
        return cls(*cls._checkpoint_args(load_checkpoint(ck)), **kw)

    def stats(self) -> dict:
        """The device state struct (one host synchronisation)."""
        return read_state(self._STATE, self.state)

    def _stream(self):
        return stream(self.device)

    def _ensure_ws(self, rows: int):
        need = int(self._ws_bytes(int(rows)))
        if self.ws.numel() < need:
            self.ws = torch.empty(need, dtype=torch.uint8, device=self.device)

    _check = staticmethod(check_tensor)


class FusedActorCritic(FusedTrainer):
    """The on-policy trainers: a policy and a value network in one vector ``[policy | value | log_std | padding]``, both aliased
    by ``.actor`` / ``.critic``.  A subclass names its widths, its key for ``log_std`` and its ``unpack``."""

    OBS_DIM, ACT_DIM = 965, 2
    _PAD = 0                 # zeros behind log_std
    LOG_STD_KEY = "log_std_parameter"
    _unpack = None           # staticmethod(unpack) of the subclass's module

    def _networks(self, policy, value, log_std) -> None:
        """``policy`` / ``value``: (descriptor, packed host array) pairs; builds the vectors, the replicas and the networks."""
        (self.desc_p, pa), (self.desc_v, pv) = policy, value
        self.P = self._param_floats(self.desc_p, self.desc_v)
        self.n_p, self.n_v = pa.size, pv.size
        ls = torch.as_tensor(log_std).detach().float().cpu().reshape(-1)
        if ls.numel() != self.ACT_DIM:
            raise ValueError(f"log_std_parameter must hold {self.ACT_DIM} values")
        flat = np.concatenate([pa, pv, ls.numpy(), np.zeros(self._PAD, np.float32)])
        assert flat.size == self.P
        self._alloc(flat)
        self.rep_p, self.actor = self._replica(self.desc_p, self.params[:self.n_p])
        self.rep_v, self.critic = self._replica(self.desc_v, self.params[self.n_p:self.n_p + self.n_v])
        self._gae_hp = default_hparams(_lib.PpoHparams, "rover_ppo_default_hparams")

    @staticmethod
    def _checkpoint_args(ck):
        return ck["policy"], ck["value"]

    @property
    def log_std(self) -> torch.Tensor:
        """The raw (unclamped) log_std parameter, a view of the device vector."""
        return self.params[self.n_p + self.n_v:self.n_p + self.n_v + self.ACT_DIM]

    def state_dict(self) -> dict:
        """``{"policy": ..., "value": ...}`` in the skrl / example layout (float32 CPU tensors)."""
        p = self.params.cpu()
        pol = self._unpack(self.desc_p, p[:self.n_p])
        pol[self.LOG_STD_KEY] = p[self.n_p + self.n_v:self.n_p + self.n_v + self.ACT_DIM].clone()
        return {"policy": pol, "value": self._unpack(self.desc_v, p[self.n_p:self.n_p + self.n_v])}

    def gae(self, rew: torch.Tensor, done: torch.Tensor, val: torch.Tensor, last_v: torch.Tensor):
        """(adv, ret) of (T, n_envs) rollouts (``rover_ppo_gae``), bit-identical to the example's torch loop; adv is not
        normalised."""
        for t, nm in ((rew, "rew"), (done, "done"), (val, "val"), (last_v, "last_v")):
            self._check(t, nm)
        h = self._gae_hp
        h.gamma, h.lam = self.hp.gamma, self.hp.lam
        T, n = rew.shape
        adv, ret = torch.empty_like(rew), torch.empty_like(rew)
        _lib.check(self._lib.rover_ppo_gae(C.byref(h), rew.data_ptr(), done.data_ptr(), val.data_ptr(), last_v.data_ptr(), T, n,
                                           adv.data_ptr(), ret.data_ptr(), self._stream()), "rover_ppo_gae")
        return adv, ret

    def _flat_rollout(self, obs, act, **rows):
        """Rollout buffers, flat (B, ...) or (T, n_envs, ...), as checked flat ones: (obs, act, the per-row ones in the order
        given, B)."""
        obs = obs.reshape(-1, obs.shape[-1])
        B = obs.shape[0]
        act = act.reshape(B, -1)
        flat = [x.reshape(B) for x in rows.values()]
        for t, nm in ((obs, "obs"), (act, "act"), *zip(flat, rows)):
            self._check(t, nm)
        if obs.shape[1] != self.OBS_DIM or act.shape[1] != self.ACT_DIM:
            raise ValueError(f"obs must be (B, {self.OBS_DIM}) and act (B, {self.ACT_DIM})")
        return (obs, act, *flat, B)

    def _minibatches(self, perms, e: int, B: int, mbs: int):
        """The minibatches of epoch ``e``: ``perms[e]``, or a fresh permutation, in ``mbs`` chunks."""
        perm = perms[e] if perms is not None else torch.randperm(B, device=self.device)
        chunks = perm.chunk(mbs)
        if len(chunks) != mbs:
            raise ValueError(f"{B} rows do not make {mbs} minibatches")
        return chunks


class FusedOffPolicy(FusedTrainer):
    """The off-policy trainers: an actor and twin critics at the head of one vector ``[actor | critic_1 | critic_2 | ...]``,
    the actor aliased by ``.actor``, and a ``td3.ReplayMemory`` as the source of every batch."""

    OBS_DIM, ACT_DIM = 965, 2
    _unpack = None           # staticmethod(ppo.unpack)

    def _networks(self, actor, critic_1, critic_2):
        """(descriptor, packed host array) pairs -> the three packed arrays; sets the descriptors, the sizes and ``P``."""
        (self.desc_a, pa), (self.desc_c, pc1), (_, pc2) = actor, critic_1, critic_2
        self.P = self._param_floats(self.desc_a, self.desc_c)
        self.n_a, self.n_c = pa.size, pc1.size
        return pa, pc1, pc2

    def _alloc(self, flat: np.ndarray) -> None:
        super()._alloc(flat)
        self.rep_a, self.actor = self._replica(self.desc_a, self.params[:self.n_a])

    def blocks(self, vec: torch.Tensor) -> dict:
        """The actor / critic_1 / critic_2 slices of a vector in this layout."""
        a, c = self.n_a, self.n_c
        return {"policy": vec[:a], "critic_1": vec[a:a + c], "critic_2": vec[a + c:a + 2 * c]}

    def unvector(self, vec: torch.Tensor) -> dict:
        """state_dict-shaped float32 CPU tensors of each network block of a vector in this layout."""
        b = {k: v.detach().cpu() for k, v in self.blocks(vec).items()}
        descs = {"policy": self.desc_a, "critic_1": self.desc_c, "critic_2": self.desc_c}
        return {k: self._unpack(descs[k], b[k]) for k in descs if k in b}

    def _sample(self, memory, idx: torch.Tensor) -> int:
        if memory.obs.device != self.params.device or not idx.is_cuda or idx.dtype != torch.int64 or not idx.is_contiguous():
            raise ValueError("idx must be a contiguous int64 cuda tensor on the memory's device")
        if memory.obs.shape[-1] != self.OBS_DIM or memory.actions.shape[-1] != self.ACT_DIM:
            raise ValueError("the memory must hold 965-wide observations and 2-wide actions")
        if len(memory) == 0:
            raise ValueError("the memory is empty")
        n = int(idx.numel())
        self._ensure_ws(n)
        return n

    @staticmethod
    def _out(t, numel: int, name: str):
        """The pointer of an optional output of ``numel`` floats (NULL for ``None``)."""
        if t is None:
            return None
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != numel:
            raise ValueError(f"{name} must be a contiguous float32 cuda tensor of {numel} floats")
        return t.data_ptr()
