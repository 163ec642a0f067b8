"""Shared cases of the policy forward tests (test_policy.py on the C oracle, test_gpu_policy_edges.py on the three HIP kernels):
a float64 restatement of the reference's two model classes, the data sets away from the friendly synthetic rows, framed output
buffers, observation rows at a chosen byte alignment, and the small network that takes the descriptor-driven kernel.

The float64 reference is written from the meaning of rover_envs/envs/navigation/learning/skrl/models.py (GaussianNeuralNetwork.compute
:89-103, DeterministicNeuralNetwork.compute :151-163) in numpy, one matrix product per Linear: it shares no text with
oracle/policy_oracle.c or with the kernels, and no summation order either.
"""
import numpy as np

from helpers import random_policy_weights, synthetic_obs

FLT_MIN = float(np.finfo(np.float32).tiny)

# ---------------------------------------------------------------------------------------------- float64 / float32 references
def reference64_generic(ws, bs, obs, n_enc, prop_dim, obs_dim, final_tanh, slope=0.01):
    """The models' compute() in float64 for any descriptor: the first ``n_enc`` Linears are the encoder on
    ``states[:, prop_dim - 1:-1]`` (models.py:95: one column early, the last column dropped), the rest the MLP on
    ``cat(states[:, :prop_dim], encoder output)`` (or on ``states[:, :prop_dim]`` alone without an encoder); LeakyReLU(slope)
    after every Linear but the last, tanh or nothing after the last."""
    s = np.asarray(obs, dtype=np.float64)
    assert s.ndim == 2 and s.shape[1] == obs_dim and len(ws) == len(bs) and 0 <= n_enc < len(ws)

    def linear(x, i):
        return x @ np.asarray(ws[i], dtype=np.float64).T + np.asarray(bs[i], dtype=np.float64)

    def leaky(x):
        return np.where(x > 0, x, slope * x)

    x = s[:, :prop_dim]
    if n_enc > 0:
        e = s[:, prop_dim - 1:-1]
        for i in range(n_enc):
            e = leaky(linear(e, i))
        x = np.concatenate([x, e], axis=1)
    for i in range(n_enc, len(ws) - 1):
        x = leaky(linear(x, i))
    x = linear(x, len(ws) - 1)
    return np.tanh(x) if final_tanh else x


def reference64(ws, bs, obs, final_tanh, slope=0.01):
    """The reference architecture: encoder on obs[:, 3:-1], cat(obs[:, :4], enc), LeakyReLU, np.tanh or nothing."""
    return reference64_generic(ws, bs, obs, 2, 4, 965, final_tanh, slope)


def torch32_generic(ws, bs, obs, n_enc, prop_dim, final_tanh, slope=0.01):
    """Plain torch fp32 on the CPU for any descriptor (helpers.torch_policy_reference is the reference architecture's)."""
    import torch
    F = torch.nn.functional
    s = torch.as_tensor(np.asarray(obs, dtype=np.float32))
    W, B = [torch.as_tensor(w) for w in ws], [torch.as_tensor(b) for b in bs]
    x = s[:, :prop_dim]
    if n_enc > 0:
        e = s[:, prop_dim - 1:-1]
        for i in range(n_enc):
            e = F.leaky_relu(F.linear(e, W[i], B[i]), slope)
        x = torch.cat([x, e], 1)
    for i in range(n_enc, len(ws) - 1):
        x = F.leaky_relu(F.linear(x, W[i], B[i]), slope)
    x = F.linear(x, W[-1], B[-1])
    return (torch.tanh(x) if final_tanh else x).numpy()


# ---------------------------------------------------------------------------------------------- data sets: f(n, seed) -> (n, 965) float32
def synthetic(n, seed):
    return synthetic_obs(n, seed)


def big(n, seed):
    return synthetic_obs(n, seed) * np.float32(1e3)


def tiny(n, seed):
    return synthetic_obs(n, seed) * np.float32(1e-20)


def cancel(n, seed):
    """Scan columns alternating +1e4, -1e4 plus 0.1 N(0, 1): the 961-wide layer sums terms 1e5 times its result's size."""
    rng = np.random.RandomState(seed)
    obs = synthetic_obs(n, seed)
    sign = np.where(np.arange(961) % 2 == 0, 1e4, -1e4)
    obs[:, 4:] = (sign[None, :] + 0.1 * rng.standard_normal((n, 961))).astype(np.float32)
    return obs


def subnormal(n, seed):
    """Every scan column below FLT_MIN in magnitude; used with all-zero biases, so that every intermediate stays there."""
    return synthetic_obs(n, seed) * np.float32(1e-38)


DATA = {"synthetic": synthetic, "big": big, "tiny": tiny, "cancel": cancel}
HARD_ROWS = (1, 17, 33)
POLICY_SEED, VALUE_SEED = 5, 4


def scaled_down_policy_head(ws, bs, obs):
    """The policy's last layer times a power of two (exact in fp32) that brings the float64 pre-activations on ``obs`` to at most
    0.5: on `big` and `cancel` the unscaled head saturates, and tanh = +-1 would compare nothing."""
    z = reference64(ws, bs, obs, final_tanh=False)
    s = np.float32(2.0 ** np.floor(np.log2(0.5 / np.abs(z).max())))
    return ws[:-1] + [ws[-1] * s], bs[:-1] + [bs[-1] * s]


def hard_cases():
    """(name, ws, bs, final_tanh, obs) of the float64 comparison: `synthetic` and `tiny` with both heads, `big` and `cancel` with the
    value head and with a policy head whose last layer is scaled down; n in HARD_ROWS; weights of scale 3."""
    out = []
    for data, f in DATA.items():
        for n in HARD_ROWS:
            obs = f(n, n)
            ws, bs = random_policy_weights(seed=VALUE_SEED, out_dim=1, scale=3.0)
            out.append((f"{data} value n={n}", ws, bs, False, obs))
            ws, bs = random_policy_weights(seed=POLICY_SEED, out_dim=2, scale=3.0)
            if data in ("big", "cancel"):
                ws, bs = scaled_down_policy_head(ws, bs, obs)
            out.append((f"{data} policy n={n}", ws, bs, True, obs))
    return out


def subnormal_case(n):
    """(ws, bs, obs): value head of scale 3, all-zero biases, `subnormal` rows.  The network's gain on these rows is about one, so a
    few outputs would reach FLT_MIN: the last layer is scaled by the power of two that keeps the float64 outputs at or below
    FLT_MIN / 2 (a property of the inputs, taken from the float64 reference)."""
    ws, bs = random_policy_weights(seed=VALUE_SEED, out_dim=1, scale=3.0)
    bs = [np.zeros_like(b) for b in bs]
    obs = subnormal(n, n)
    z = np.abs(reference64(ws, bs, obs, False)).max()
    s = np.float32(2.0 ** min(0.0, np.floor(np.log2(0.5 * FLT_MIN / z))))
    return ws[:-1] + [ws[-1] * s], bs, obs


# ---------------------------------------------------------------------------------------------- the small generic networks
# test_gpu_policy.py::test_generic_architectures' second network: K and N ragged on every layer, the descriptor-driven kernel
SMALL_SHAPES = [(20, 64), (9, 20), (50, 15), (3, 50)]
SMALL = dict(n_enc=2, obs_dim=70, prop_dim=6, final_act="tanh")
# MLP only; its last layer is full-K: the N guard, the row guard and the global store in one epilogue
MLP_SHAPES = [(33, 10), (7, 33)]
MLP = dict(n_enc=0, obs_dim=10, prop_dim=10, final_act="none")
# MLP only; its last layer is split-K (one column tile, K >= 128) with a ragged K: the split-K combine as the global store
SPLIT_SHAPES = [(130, 10), (3, 130)]
SPLIT = dict(n_enc=0, obs_dim=10, prop_dim=10, final_act="tanh")


def random_weights(shapes, seed):
    rng = np.random.RandomState(seed)
    ws = [(rng.uniform(-1, 1, s) / np.sqrt(s[1]) * 2.0).astype(np.float32) for s in shapes]
    bs = [(rng.uniform(-1, 1, (s[0],)) * 0.1).astype(np.float32) for s in shapes]
    return ws, bs


def normal_obs(n, obs_dim, seed):
    return np.random.RandomState(seed).standard_normal((n, obs_dim)).astype(np.float32)


# ---------------------------------------------------------------------------------------------- one bad row in a tile
BAD_VALUES = (float("nan"), float("inf"), float("-inf"), 3e38)
BAD_N, BAD_ROWS = 33, (5, 32)    # row 5 of tile 0 and row 0 of tile 2 (a ragged tile of one row)


def bad_columns(prop_dim, obs_dim):
    """The MLP's first and last proprioceptive column (the last is the encoder's first input too), the encoder's second input,
    its last input, and the column nothing reads."""
    return (0, prop_dim - 1, prop_dim, obs_dim - 2, obs_dim - 1)


def with_bad(obs, col, value, rows=BAD_ROWS):
    out = obs.copy()
    out[list(rows), col] = np.float32(value)
    return out


def bits_equal(a, b):
    """numpy float32 arrays equal on every bit."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def bits_equal_nan_aware(a, b):
    """NaN at the same places, whatever its payload, and every other element equal on the bits (td3_helpers.same_bits_nan_aware
    for numpy arrays)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb])


# ---------------------------------------------------------------------------------------------- device buffers
FRAME_BITS = 0x7FC0BEEF          # a quiet NaN with a payload no arithmetic produces
FRAME_ROWS = 16                  # a whole tile written past row n still lands in the frame, inside the allocation


def _words(count, device):
    import torch
    return torch.full((count,), FRAME_BITS, dtype=torch.int32, device=device).view(torch.float32)


def framed(n, out_dim, byte_offset=4, device="cuda"):
    """(whole buffer, contiguous (n, out_dim) view, index of the view's first float): at least FRAME_ROWS rows of FRAME_BITS words
    on either side; the view's first byte lies ``byte_offset`` (0, 4, 8, 12) past a 16-byte boundary of the allocation."""
    assert byte_offset % 4 == 0 and 0 <= byte_offset < 16
    guard = (FRAME_ROWS * out_dim + 3) // 4 * 4
    start = guard + byte_offset // 4
    whole = _words(start + n * out_dim + guard + 4, device)
    assert whole.data_ptr() % 16 == 0
    view = whole[start:start + n * out_dim].view(n, out_dim)
    assert view.is_contiguous() and view.data_ptr() % 16 == byte_offset
    return whole, view, start


def frame_intact(whole, view, start):
    import torch
    raw = whole.view(torch.int32)
    return bool((raw[:start] == FRAME_BITS).all()) and bool((raw[start + view.numel():] == FRAME_BITS).all())


def obs_at(obs, byte_offset, device="cuda"):
    """The rows of ``obs`` (numpy or tensor, (n, w) float32) in a larger device buffer of FRAME_BITS words, as a contiguous view
    whose first byte lies ``byte_offset`` past a 16-byte boundary."""
    import torch
    assert byte_offset % 4 == 0 and 0 <= byte_offset < 16
    src = torch.as_tensor(obs)
    n, w = src.shape
    lead = 4 + byte_offset // 4
    whole = _words(lead + n * w + 8, device)
    assert whole.data_ptr() % 16 == 0
    view = whole[lead:lead + n * w].view(n, w)
    view.copy_(src)
    assert view.is_contiguous()
    return view
