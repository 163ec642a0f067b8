"""The host plumbing the fused trainers share (``isaac_rover_orbit_amd._fused``), as far as it runs without a GPU: the hparams
overrides, pack / unpack (``rover_policy_pack`` / ``rover_policy_unpack`` are host functions), checkpoints and the state reader.

``tests/golden/fused_host_packed.json`` holds the sha256 of each packed buffer below as the code BEFORE the shared module produced
it from the same weights (the buffers themselves, 2.4 MB of incompressible floats, exceed the size of a committed file).  The
weights come from ``numpy.random.RandomState``, whose streams are frozen, not from torch's initialisers."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_host_packed.json")
ENC, MLP, LIFT = "dense_encoder.encoder_layers.{}.{}", "mlp.{}.{}", "net.{}.{}"


def _sd(rng, groups):
    """state_dict of Linear layers: ``groups`` pairs (key pattern, [(out, in), ...]), Linear i of a group at index 2 i."""
    sd = {}
    for pat, shapes in groups:
        for i, (n, k) in enumerate(shapes):
            sd[pat.format(2 * i, "weight")] = torch.from_numpy(rng.standard_normal((n, k)).astype(np.float32) / np.float32(np.sqrt(k)))
            sd[pat.format(2 * i, "bias")] = torch.from_numpy(rng.standard_normal(n).astype(np.float32) * np.float32(0.1))
    return sd


def state_dicts():
    """Seeded weights in the five layouts: rover actor (``Net(2, True)``), rover critic, ``td3.Critic``, lift policy, lift value."""
    rng = np.random.RandomState(20261019)
    enc = [(80, 961), (60, 80)]
    rover = lambda first, out: [(ENC, enc), (MLP, [(256, first), (160, 256), (128, 160), (out, 128)])]  # noqa: E731
    lift = lambda out: [(LIFT, [(256, 36), (128, 256), (64, 128), (out, 64)])]  # noqa: E731
    return {"rover_actor": _sd(rng, rover(64, 2)), "rover_critic": _sd(rng, rover(64, 1)), "td3_critic": _sd(rng, rover(66, 1)),
            "lift_policy": _sd(rng, lift(8)), "lift_value": _sd(rng, lift(1))}


def packers():
    from isaac_rover_orbit_amd import lift_ppo, ppo, td3
    return {"rover_actor": (lambda sd: ppo.pack(sd, "tanh"), ppo.unpack), "rover_critic": (lambda sd: ppo.pack(sd, "none"), ppo.unpack),
            "td3_critic": (td3.pack_critic, ppo.unpack), "lift_policy": (lift_ppo.pack, lift_ppo.unpack),
            "lift_value": (lift_ppo.pack, lift_ppo.unpack)}


def packed_digests() -> dict:
    return {k: hashlib.sha256(packers()[k][0](sd)[1].tobytes()).hexdigest() for k, sd in state_dicts().items()}


@pytest.fixture(scope="module")
def sds():
    return state_dicts()


# ------------------------------------------------------------------------------------------------------------------- hparams
def _hparam_cases():
    from isaac_rover_orbit_amd import lift_ppo, ppo, sac, td3, trpo
    return [(ppo, "gamma"), (lift_ppo, "reward_scale"), (trpo, "damping"), (td3, "polyak"), (sac, "entropy_lr")]


@pytest.mark.parametrize("i", range(5))
def test_set_hparams_sets_refuses_and_converts(i):
    from isaac_rover_orbit_amd import _fused, sac
    mod, field = _hparam_cases()[i]
    hp = mod.default_hparams()
    assert _fused.set_hparams(hp, {field: 0.125}) is hp and getattr(hp, field) == 0.125
    with pytest.raises(TypeError, match="unknown hyper-parameter 'nope'"):
        _fused.set_hparams(hp, {"nope": 1})
    if mod is sac:
        convert = {"learn_entropy": lambda v: int(bool(v))}
        assert _fused.set_hparams(hp, {"learn_entropy": True}, convert).learn_entropy == 1
        assert _fused.set_hparams(hp, {"learn_entropy": False}, convert).learn_entropy == 0


def test_default_hparams_is_the_librarys():
    from isaac_rover_orbit_amd import _fused, _lib, td3
    a, b = _fused.default_hparams(_lib.Td3Hparams, "rover_td3_default_hparams"), td3.default_hparams()
    assert bytes(a) == bytes(b) and isinstance(b, _lib.Td3Hparams)


# -------------------------------------------------------------------------------------------------------------- pack / unpack
@pytest.mark.parametrize("name", ["rover_actor", "rover_critic", "td3_critic", "lift_policy", "lift_value"])
def test_pack_unpack_round_trip_is_bit_exact(sds, name):
    pack, unpack = packers()[name]
    sd = sds[name]
    desc, packed = pack(sd)
    assert packed.dtype == np.float32 and packed.ndim == 1
    back = unpack(desc, packed)
    assert list(back) == list(sd)                                  # the same keys in the same order
    for k, v in sd.items():
        assert back[k].dtype == torch.float32 and back[k].shape == v.shape
        assert torch.equal(back[k].view(torch.int32), v.view(torch.int32)), k
    assert np.array_equal(pack(back)[1].view(np.int32), packed.view(np.int32))


def test_packed_buffers_are_those_of_the_code_before_the_shared_module():
    with open(GOLDEN) as f:
        want = json.load(f)
    assert packed_digests() == want


def test_pack_refusals_stay():
    from isaac_rover_orbit_amd import lift_ppo, td3
    sds_ = state_dicts()
    with pytest.raises(ValueError, match="no net.<i>.weight entries"):
        lift_ppo.pack(sds_["rover_actor"])
    with pytest.raises(ValueError, match="not a Critic state_dict"):
        td3.pack_critic(sds_["lift_value"])


# ------------------------------------------------------------------------------------------------------- checkpoints, state
def test_load_checkpoint_takes_a_path_or_the_dict(tmp_path, sds):
    from isaac_rover_orbit_amd import _fused
    ck = {"policy": sds["lift_policy"], "value": sds["lift_value"], "step": 7}
    path = str(tmp_path / "ck.pt")
    torch.save(ck, path)
    assert _fused.load_checkpoint(ck) is ck
    got = _fused.load_checkpoint(path)
    assert list(got) == list(ck) and got["step"] == 7
    for part in ("policy", "value"):
        assert list(got[part]) == list(ck[part]) and all(torch.equal(got[part][k], v) for k, v in ck[part].items())


def test_read_state_leaves_out_the_reserved_fields():
    from isaac_rover_orbit_amd import _fused, _lib
    for cls in (_lib.TrpoState, _lib.Td3State, _lib.SacState):
        raw = np.arange(C.sizeof(cls) // 4, dtype=np.int32)
        got = _fused.read_state(cls, torch.from_numpy(raw))
        names = [f for f, *_ in cls._fields_]
        assert [n for n in names if n.startswith("reserved")], cls           # each of them has padding to leave out
        assert list(got) == [n for n in names if not n.startswith("reserved")]
        st = cls.from_buffer_copy(raw.tobytes())
        assert all(got[k] == getattr(st, k) for k in got)
    trpo = _fused.read_state(_lib.TrpoState, torch.zeros(C.sizeof(_lib.TrpoState) // 4, dtype=torch.int32))
    assert not {"reserved0", "reserved1"} & set(trpo)
    assert {"reserved0", "reserved1"} <= {f for f, *_ in _lib.TrpoState._fields_}
    assert "reserved" in {f for f, *_ in _lib.Td3State._fields_} and "reserved" in {f for f, *_ in _lib.SacState._fields_}


def test_require_gpu_keeps_each_callers_wording(monkeypatch):
    from isaac_rover_orbit_amd import _fused, _lib
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.RoverHipError, match=r"^FusedPPO needs a ROCm GPU \(no CPU fallback\)$"):
        _fused.require_gpu("FusedPPO")
    with pytest.raises(_lib.RoverHipError,
                       match=r"^RolloutCollector needs a ROCm GPU \(no CPU fallback; TorchRollout is the CPU specification\)$"):
        _fused.require_gpu("RolloutCollector", "TorchRollout is the CPU specification")



# ------------------------------------------------------------------------------------------------------------------- row pitch
def _layout(t, width, rows=None):
    from isaac_rover_orbit_amd import _fused
    return _fused.layout_pitch(tuple(t.shape), t.stride(), t.is_contiguous(), width, rows)


def test_row_pitch_is_one_rule_for_padded_rows_and_contiguous_images():
    """``_fused.row_pitch``: the layout half on CPU tensors' own shapes and strides, the dtype / device half as far as it runs
    without a GPU, and the whole of it on the device where there is one."""
    from isaac_rover_orbit_amd import _fused
    base = torch.zeros(64)
    strided = lambda shape, stride: base.as_strided(shape, stride)      # noqa: E731
    # accepted: plain rows, a padded pitch, one row with any row stride, a contiguous image
    assert _layout(torch.zeros(3, 6), 6) == 6 and _layout(torch.zeros(3, 6), 6, rows=3) == 6
    assert _layout(strided((3, 6), (10, 1)), 6) == 10 and _layout(torch.zeros(3, 10)[:, 2:8], 6) == 10
    assert _layout(strided((1, 6), (2, 1)), 6) == 6 and _layout(strided((1, 6), (40, 1)), 6, rows=1) == 6
    assert _layout(torch.zeros(3, 2, 3), 6) == 6 and _layout(torch.zeros(3, 2, 3), 6, rows=3) == 6
    assert _layout(torch.zeros(0, 6), 6) == 6
    # refused: rows that overlap, a column stride of 2, a wrong width, a wrong row count, one dimension, a permuted image
    assert _layout(strided((3, 6), (4, 1)), 6) is None
    assert _layout(strided((3, 6), (12, 2)), 6) is None and _layout(strided((1, 6), (12, 2)), 6) is None
    assert _layout(torch.zeros(3, 6), 5) is None and _layout(torch.zeros(3, 6), 7) is None and _layout(torch.zeros(3, 2, 3), 5) is None
    assert _layout(torch.zeros(3, 6), 6, rows=2) is None and _layout(torch.zeros(3, 2, 3), 6, rows=4) is None
    assert _layout(torch.zeros(6), 6) is None and _layout(torch.zeros(6), 6, rows=6) is None and _layout(torch.zeros(1), 1, rows=1) is None
    assert _layout(torch.zeros(3, 3, 2).permute(0, 2, 1), 6) is None
    for bad in (torch.zeros(3, 6), np.zeros((3, 6), np.float32), None):           # not on the device: refused by name
        with pytest.raises(ValueError, match="^scan_out must be a float32 cuda tensor"):
            _fused.row_pitch("scan_out", bad, 6)
    if not torch.cuda.is_available():
        return
    dev = torch.device("cuda", torch.cuda.current_device())
    pad = torch.zeros(3, 10, device=dev)
    assert _fused.row_pitch("rows", pad[:, :6], 6, rows=3, device=dev) == 10 and _fused.row_pitch("rows", pad[:1, 4:], 6) == 6
    assert _fused.row_pitch("rows", torch.zeros(3, 2, 3, device=dev), 6) == 6
    for bad, kw in ((pad[:, ::2], {}), (pad[:, :6], {"rows": 4}), (pad[0, :6], {}), (pad.double()[:, :6], {}), (pad[:, :5], {}),
                    (pad[:, :6], {"device": torch.device("cpu")})):
        with pytest.raises(ValueError, match="^depth must "):
            _fused.row_pitch("depth", bad, 6, **kw)
