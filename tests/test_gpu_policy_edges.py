"""The policy forward pass (include/rover_policy.h) at tile edges, alignments, bad rows, replicas and hard data, in all three
kernel bodies:

  * reference -- the reference architecture through RoverNet (rover_policy_ref_kernel);
  * pair      -- the reference architecture through forward_pair (rover_policy_ref_pair_kernel): a policy head and a value head;
  * generic   -- policy_cases.SMALL, K and N ragged on every layer (rover_policy_kernel, descriptor-driven).

Bit comparisons (td3_helpers.same_bits_nan_aware) are against the C oracle, whose chains, split-K cuts and tanh sequence are the
header's contract; values are compared with a numpy float64 restatement of models.py under the project's own rule
(td3_helpers.check: the error norm within 4 x torch fp32's, plus 1e-5 of the reference's norm).  Outputs go into framed buffers
where the test is about rows: a store past row n lands in the frame and is seen.
"""
import numpy as np
import pytest
import torch

import policy_cases as pc
from helpers import random_policy_weights, synthetic_obs, torch_policy_reference
from td3_helpers import check, err, same_bits_nan_aware

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def po():
    from oracle import policy_oracle
    policy_oracle.build()
    return policy_oracle


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want):
    """A device tensor against a numpy array of the oracle, on the bits."""
    return same_bits_nan_aware(got.detach().cpu(), torch.from_numpy(np.ascontiguousarray(want)))


class Member:
    """One network: its weights, what describes it to the references, and the RoverNet that runs it."""

    def __init__(self, ws, bs, n_enc=2, obs_dim=965, prop_dim=4, final_act="tanh", net=None):
        from isaac_rover_orbit_amd.policy import RoverNet
        self.ws, self.bs, self.n_enc, self.obs_dim, self.prop_dim, self.final_tanh = ws, bs, n_enc, obs_dim, prop_dim, final_act == "tanh"
        self.net = net or RoverNet(ws, bs, n_enc=n_enc, final_act=final_act, obs_dim=obs_dim, prop_dim=prop_dim)
        self.out_dim = self.net.out_dim

    def oracle(self, po, obs):
        return po.forward(po.desc_from(self.net.desc), self.ws, self.bs, obs)

    def torch32(self, obs):
        return pc.torch32_generic(self.ws, self.bs, obs, self.n_enc, self.prop_dim, self.final_tanh)


class Family:
    """What one launch evaluates: one network, or an actor and a critic through forward_pair."""

    def __init__(self, members, pair=False):
        self.members, self.pair = members, pair
        self.obs_dim, self.prop_dim = members[0].obs_dim, members[0].prop_dim
        self.out_dims = [m.out_dim for m in members]

    def run(self, obs, outs=None):
        from isaac_rover_orbit_amd.policy import forward_pair
        if self.pair:
            a, b = self.members
            got = forward_pair(a.net, b.net, obs, *(outs or (None, None)))
        else:
            got = (self.members[0].net(obs, outs[0] if outs else None),)
        torch.cuda.synchronize()
        return got

    def oracle(self, po, obs):
        return [m.oracle(po, obs) for m in self.members]

    def rows(self, n, seed):
        return synthetic_obs(n, seed) if self.obs_dim == 965 else pc.normal_obs(n, self.obs_dim, seed)


_FAMILIES = {}


def family(kind):
    """reference / pair (actor of 2) / pair6 (actor of 6, the wide head) / generic / generic-mlp (full-K last layer) / generic-split
    (split-K last layer), built once."""
    if kind not in _FAMILIES:
        if kind == "reference":
            fam = Family([Member(*random_policy_weights(seed=31, out_dim=2, scale=3.0))])
        elif kind in ("pair", "pair6"):
            fam = Family([Member(*random_policy_weights(seed=32, out_dim=6 if kind == "pair6" else 2, scale=3.0)),
                          Member(*random_policy_weights(seed=33, out_dim=1, scale=3.0), final_act="none")], pair=True)
        elif kind == "generic":
            fam = Family([Member(*pc.random_weights(pc.SMALL_SHAPES, seed=34), **pc.SMALL)])
        elif kind == "generic-mlp":
            fam = Family([Member(*pc.random_weights(pc.MLP_SHAPES, seed=35), **pc.MLP)])
        else:
            fam = Family([Member(*pc.random_weights(pc.SPLIT_SHAPES, seed=36), **pc.SPLIT)])
            assert [fam.members[0].net.desc.layers[i].split_k for i in range(2)] == [0, 1]
        _FAMILIES[kind] = fam
    return _FAMILIES[kind]


THREE = ("reference", "pair", "generic")


def test_the_cases_reach_the_kernels_they_name(monkeypatch):
    """The pair cases take rover_policy_forward_pair itself, not the binding's two-launch path for other architectures, and the small
    networks are not the reference architecture (rover_policy_forward gives those to the descriptor-driven kernel)."""
    from isaac_rover_orbit_amd.policy import RoverNet

    def two_launches(*a, **k):
        raise AssertionError("forward_pair fell back to two rover_policy_forward launches")
    for kind in ("pair", "pair6"):
        fam = family(kind)
        obs = _dev(fam.rows(17, 1))
        with monkeypatch.context() as m:
            m.setattr(RoverNet, "__call__", two_launches)
            fam.run(obs)
    for kind in ("generic", "generic-mlp", "generic-split"):
        d = family(kind).members[0].net.desc
        assert (d.obs_dim, d.n_enc + d.n_mlp) != (965, 6)


# ------------------------------------------------------------------------------------------------ (a) rows around the tile
@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 32, 33, 47])
@pytest.mark.parametrize("kind", ["reference", "pair", "pair6", "generic", "generic-mlp", "generic-split"])
def test_rows_around_the_tile_and_nothing_outside(po, kind, n):
    """One short of a tile, a tile, one into the next, two tiles and around them: bit-equal to the oracle, and the 16 rows of frame
    on either side of every output keep every word.  The outputs start 4 bytes off a 16-byte boundary.  The kinds reach the four
    epilogues that store to global memory: the two layer-6 combines, the generic kernel's full-K store and its split-K combine."""
    fam = family(kind)
    obs = fam.rows(n, seed=100 + n)
    frames = [pc.framed(n, d, byte_offset=4) for d in fam.out_dims]
    views = [f[1] for f in frames]
    assert all(v.data_ptr() % 16 == 4 and v.is_contiguous() for v in views)
    got = fam.run(_dev(obs), views)
    for g, v, frame, want, d in zip(got, views, frames, fam.oracle(po, obs), fam.out_dims):
        assert g is v and g.shape == (n, d)
        assert pc.frame_intact(*frame), f"{kind}, n = {n}: a word outside the ({n}, {d}) output was written"
        assert _same(g, want), f"{kind}, n = {n}, out_dim {d}"


# ------------------------------------------------------------------------------------------------ (b) both staging paths
@pytest.mark.parametrize("n", [16, 32, 17])
@pytest.mark.parametrize("kind", THREE)
def test_both_staging_paths_at_every_alignment(po, kind, n):
    """The observation block 0, 4, 8 and 12 bytes off a 16-byte boundary: at 0 full tiles take the 16-byte loads (or LDS-DMA) and the
    17th row the scalar copy, elsewhere every tile takes the scalar copy -- the same bits every time, the oracle's."""
    fam = family(kind)
    obs = fam.rows(n, seed=200 + n)
    want = fam.oracle(po, obs)
    results = []
    for off in (0, 4, 8, 12):
        o = pc.obs_at(obs, off)
        assert o.data_ptr() % 16 == off and o.is_contiguous() and o.shape == obs.shape
        assert torch.equal(o.cpu(), torch.from_numpy(obs))
        got = fam.run(o)
        for g, w in zip(got, want):
            assert _same(g, w), f"{kind}, n = {n}, {off} bytes off"
        results.append(got)
    for got in results[1:]:
        for g, g0 in zip(got, results[0]):
            assert same_bits_nan_aware(g, g0)


# ------------------------------------------------------------------------------------------------ (c) one bad row in a tile
@pytest.mark.parametrize("kind", THREE)
def test_one_bad_row_in_a_tile(po, kind):
    """n = 33; row 5 of tile 0 and row 0 of tile 2 carry a NaN, +inf, -inf or 3e38 in one column.  The rows of an MFMA tile do not
    mix: every other row keeps the clean run's bits; the bad rows are the oracle's (NaN-aware) and have a NaN wherever torch fp32
    on the CPU has one.  The last column is read by nothing (models.py:95 drops the last ray): the kernels mask it in the ragged last
    k group of the encoder's first layer, so there even the bad rows keep the clean bits -- a kernel that multiplied it by the packed
    zero would turn an infinite last ray into a NaN action."""
    fam = family(kind)
    obs = fam.rows(pc.BAD_N, seed=300)
    clean = [g.clone() for g in fam.run(_dev(obs))]
    assert all(bool(torch.isfinite(c).all()) for c in clean)
    bad_rows = list(pc.BAD_ROWS)
    others = [r for r in range(pc.BAD_N) if r not in pc.BAD_ROWS]
    for col in pc.bad_columns(fam.prop_dim, fam.obs_dim):
        for value in pc.BAD_VALUES:
            what = f"{kind}, column {col}, {value}"
            bad = pc.with_bad(obs, col, value)
            got = fam.run(_dev(bad))
            for g, c in zip(got, clean):
                assert same_bits_nan_aware(g[others], c[others]), what + ": a clean row changed"
            if col == fam.obs_dim - 1:
                for g, c in zip(got, clean):
                    assert same_bits_nan_aware(g, c), what + ": the last column was read"
                continue
            for g, m in zip(got, fam.members):
                assert _same(g[bad_rows], m.oracle(po, bad[bad_rows])), what + ": bad rows against the oracle"
                nan32 = torch.from_numpy(np.isnan(m.torch32(bad[bad_rows])))
                assert bool(torch.isnan(g[bad_rows].cpu())[nan32].all()), what + ": torch fp32 has a NaN the kernel has not"


@pytest.mark.parametrize("kind", THREE)
def test_the_last_column_of_row_15_does_not_reach_row_16(kind):
    """Row 15's ragged k group lies next to row 16's first columns in memory and in LDS.  Row 15 carries the bad value in the last
    column, row 16 a NaN in column 0 at the same time: row 15 (and every row but 16) must be the clean run's."""
    fam = family(kind)
    obs = fam.rows(pc.BAD_N, seed=301)
    clean = [g.clone() for g in fam.run(_dev(obs))]
    keep = [r for r in range(pc.BAD_N) if r != 16]
    for value in pc.BAD_VALUES:
        bad = pc.with_bad(obs, fam.obs_dim - 1, value, rows=(15,))
        bad[16, 0] = np.nan
        for off in (0, 4):                        # the wide copy and the scalar one
            o = pc.obs_at(bad, off)
            assert o.data_ptr() % 16 == off
            for g, c in zip(fam.run(o), clean):
                assert same_bits_nan_aware(g[keep], c[keep]), f"{kind}, {value}, {off} bytes off"
                assert same_bits_nan_aware(g[15], c[15]) and bool(torch.isnan(g[16]).all()), f"{kind}, {value}, {off} bytes off"


# ------------------------------------------------------------------------------------------------ (d) replicas
def _three_replicas(shapes_or_out_dim, seeds, final_act, **desc):
    """Three different networks of one shape as the three replicas of ONE RoverNet.from_packed: (that network as a Member whose
    references are never used, the three Members).  RoverNet with n_copies = 1 packs each vector; their offsets are equal."""
    from isaac_rover_orbit_amd.policy import RoverNet
    singles = []
    for s in seeds:
        ws, bs = (random_policy_weights(seed=s, out_dim=shapes_or_out_dim, scale=3.0) if isinstance(shapes_or_out_dim, int)
                  else pc.random_weights(shapes_or_out_dim, seed=s))
        net = RoverNet(ws, bs, final_act=final_act, n_copies=1, **desc)
        singles.append(Member(ws, bs, final_act=final_act, net=net, **desc))
    first = singles[0].net
    per = first.packed.numel() // first.n_copies
    for m in singles[1:]:
        for i in range(first.desc.n_enc + first.desc.n_mlp):
            assert (m.net.desc.layers[i].w_off, m.net.desc.layers[i].b_off) == (first.desc.layers[i].w_off, first.desc.layers[i].b_off)
    vecs = [m.net.packed[:per] for m in singles]
    assert not torch.equal(vecs[0], vecs[1]) and not torch.equal(vecs[1], vecs[2]) and not torch.equal(vecs[0], vecs[2])
    buf = torch.cat(vecs).contiguous()
    three = RoverNet.from_packed(first.desc, buf, 3)
    assert three.n_copies == 3 and three.packed.numel() == 3 * per
    return Member(singles[0].ws, singles[0].bs, final_act=final_act, net=three, **desc), singles, per


@pytest.mark.parametrize("kind", THREE)
def test_workgroup_b_reads_replica_b_mod_n_copies(po, kind):
    """Three DIFFERENT networks as the three replicas; n = 16 * 7 + 5 is eight workgroups: the rows of workgroup b are network
    b % 3's, on the bits.  In the pair the actor has six outputs and the critic one, so their replica strides differ (the padded
    last biases are 8 and 4 floats): a critic read at the actor's stride is another network's bytes."""
    n = 16 * 7 + 5
    if kind == "generic":
        packs = [_three_replicas(pc.SMALL_SHAPES, (41, 42, 43), **pc.SMALL)]
    elif kind == "reference":
        packs = [_three_replicas(2, (44, 45, 46), "tanh")]
    else:
        packs = [_three_replicas(6, (47, 48, 49), "tanh"), _three_replicas(1, (50, 51, 52), "none")]
        assert packs[0][2] != packs[1][2] and packs[0][2] - packs[1][2] == 4
    fam = Family([p[0] for p in packs], pair=kind == "pair")
    obs = fam.rows(n, seed=400)
    got = fam.run(_dev(obs))
    for g, (_, singles, _) in zip(got, packs):
        want = np.empty(tuple(g.shape), np.float32)
        for b in range((n + 15) // 16):
            rows = slice(16 * b, min(16 * b + 16, n))
            want[rows] = singles[b % 3].oracle(po, obs[rows])
        for b in range((n + 15) // 16):
            rows = slice(16 * b, min(16 * b + 16, n))
            assert _same(g[rows], want[rows]), f"{kind}: workgroup {b} did not read replica {b % 3}"
        # the three networks differ where it shows: replica 0's results are not the answer for the other workgroups
        assert not _same(g[16:48], singles[0].oracle(po, obs[16:48]))


# ------------------------------------------------------------------------------------------------ (e) float64 on hard data
def test_within_the_rule_against_float64_on_hard_data(po):
    """`synthetic`, `big`, `tiny`, `cancel` at n = 1, 17, 33, weights of scale 3 (policy_cases.hard_cases), each head alone and the two
    of a data set and row count through forward_pair: the kernels' error norm against numpy float64 within 4 x torch fp32's on the
    CPU plus 1e-5 of the reference's norm (td3_helpers.check, its defaults).  A policy head whose outputs saturate compares nothing:
    more than half of them lie strictly inside (-0.99, 0.99)."""
    from isaac_rover_orbit_amd.policy import RoverNet, forward_pair
    cases = pc.hard_cases()
    nets = {}
    for name, ws, bs, final_tanh, obs in cases:
        net = RoverNet(ws, bs, n_enc=2, final_act="tanh" if final_tanh else "none")
        got = net(_dev(obs)).cpu()
        r64 = torch.from_numpy(pc.reference64(ws, bs, obs, final_tanh))
        t32 = torch.from_numpy(torch_policy_reference(ws, bs, obs, final_tanh))
        print(f"{name}: fused err {err(got, r64):.3e} torch fp32 err {err(t32, r64):.3e} norm {float(r64.norm()):.3e}")
        if final_tanh:
            assert float((got.abs() < 0.99).float().mean()) > 0.5, f"{name}: a saturated head compares nothing"
        check(got, r64, t32, what=name)
        assert _same(got, po.forward(po.desc_from(net.desc), ws, bs, obs)), name
        nets[name] = (net, got, obs)
    for name in nets:                             # "<data> value n=<n>" and "<data> policy n=<n>" share their rows
        if " value " in name:
            (critic, v, obs), (actor, a, _) = nets[name], nets[name.replace(" value ", " policy ")]
            a2, v2 = forward_pair(actor, critic, _dev(obs))
            assert same_bits_nan_aware(a2.cpu(), a) and same_bits_nan_aware(v2.cpu(), v), name


@pytest.mark.parametrize("n", pc.HARD_ROWS)
def test_subnormal_rows_are_neither_flushed_nor_widened(po, n):
    """Rows of 1e-38 through zero biases and the value head: every product and every sum is a subnormal.  The f32 MFMA neither
    flushes nor widens and the header's contract is a k-ordered fmaf chain, so the result is the oracle's on the bits (derived, not
    measured), in both kernels of the reference architecture; every output nonzero and below FLT_MIN in magnitude."""
    from isaac_rover_orbit_amd.policy import RoverNet, forward_pair
    ws, bs, obs = pc.subnormal_case(n)
    net = RoverNet(ws, bs, n_enc=2, final_act="none")
    want = po.forward(po.desc_from(net.desc), ws, bs, obs)
    got = net(_dev(obs))
    other = RoverNet(*random_policy_weights(seed=pc.POLICY_SEED, out_dim=2, scale=3.0), n_enc=2, final_act="tanh")
    _, got_pair = forward_pair(other, net, _dev(obs))
    for g in (got, got_pair):
        assert bool((g != 0).all()) and bool((g.abs() < pc.FLT_MIN).all()), g.flatten()[:4]
        assert _same(g, want), (g.flatten()[:4], want.flatten()[:4])


# ------------------------------------------------------------------------------------------------ (f) out= refusals
def _refused(n, d):
    """Buffers a kernel that writes n * d contiguous floats must never be handed: wrong row count, wrong width, float64, a column
    slice of a wider tensor, a CPU tensor."""
    return {"rows": torch.zeros(n + 1, d, device="cuda"), "fewer rows": torch.zeros(n - 1, d, device="cuda"),
            "width": torch.zeros(n, d + 1, device="cuda"), "float64": torch.zeros(n, d, dtype=torch.float64, device="cuda"),
            "column slice": torch.zeros(n, d + 2, device="cuda")[:, 1:1 + d], "cpu": torch.zeros(n, d)}


def test_out_buffers_are_checked_before_any_launch(monkeypatch):
    from isaac_rover_orbit_amd.policy import RoverNet, forward_pair
    n = 20
    fam = family("pair6")
    actor, critic = (m.net for m in fam.members)
    obs = _dev(fam.rows(n, seed=500))
    launches = []
    lib = actor._lib

    class Counting:
        """The library with its two policy entries counted; everything else passes through."""

        def __getattr__(self, name):
            f = getattr(lib, name)
            if name in ("rover_policy_forward", "rover_policy_forward_pair"):
                def counted(*a):
                    launches.append(name)
                    return f(*a)
                return counted
            return f
    with monkeypatch.context() as m:
        m.setattr(actor, "_lib", Counting())
        m.setattr(critic, "_lib", Counting())
        for name, bad in _refused(n, 6).items():
            with pytest.raises(ValueError):
                actor.forward(obs, out=bad)
            with pytest.raises(ValueError):
                forward_pair(actor, critic, obs, out_a=bad)
        for name, bad in _refused(n, 1).items():
            with pytest.raises(ValueError):
                critic(obs, bad)
            with pytest.raises(ValueError):
                forward_pair(actor, critic, obs, out_b=bad)
            with pytest.raises(ValueError):
                forward_pair(actor, critic, obs, out_a=torch.empty(n, 6, device="cuda"), out_b=bad)
        torch.cuda.synchronize()
        assert launches == [], launches
        # a correct framed view is taken, written and handed back as the same object
        fa, fb = pc.framed(n, 6), pc.framed(n, 1)
        assert actor.forward(obs, out=fa[1]) is fa[1]
        want_a = fa[1].clone()
        fa2 = pc.framed(n, 6)
        got_a, got_b = forward_pair(actor, critic, obs, out_a=fa2[1], out_b=fb[1])
        torch.cuda.synchronize()
        assert got_a is fa2[1] and got_b is fb[1]
        assert launches == ["rover_policy_forward", "rover_policy_forward_pair"]
    assert same_bits_nan_aware(got_a, want_a) and same_bits_nan_aware(got_b, critic(obs))
    assert pc.frame_intact(*fa) and pc.frame_intact(*fa2) and pc.frame_intact(*fb)
