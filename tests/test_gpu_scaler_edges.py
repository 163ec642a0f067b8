"""The running scaler's kernels (csrc/scaler_kernels.hip) at second passes, ragged column blocks and hard data, against the CPU:

  * rover_scaler_train leaves the BITS of the header's reduction order restated in float64 numpy (scaler_cases.ordered_train) in all
    2 w + 1 doubles: the build has contraction off, so every float64 operation is one correctly rounded IEEE operation.  Widths
    around the 64-column blocks of the partial sums and the 256-column blocks of the mean kernel, rows around the 64-row chunks,
    columns with |mean| / sd up to 1e8, blocks preloaded with count 1e4 and 2**40
  * a NaN, +inf or -inf cell spoils its own column only
  * the gated twin: an open gate gives the ungated call's bits, a set one leaves the block and the workspace alone
  * forward / inverse / sanitise / idx on blocks whose (float)var is 0, subnormal, FLT_MAX or inf, against the fp32 oracle on the CPU
  * scaler_apply_kernel's second grid-stride pass (more than 8192 spans), with and without idx, aligned and one float off

Every input is made on the CPU and copied to the device."""
import numpy as np
import pytest
import torch

import scaler_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 777.0


def _scaler(w, block=None, **kw):
    from isaac_rover_orbit_amd.scaler import DeviceScaler
    sc = DeviceScaler(w, DEV, **kw)
    if block is not None:
        sc.block.copy_(torch.from_numpy(np.asarray(block, np.float64)))
    return sc


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def block_of(sc):
    return sc.block.cpu().numpy()


def assert_block_bits(got, want, w, what):
    if SC.same_bits64(got, want):
        return
    with np.errstate(all="ignore"):
        fin = np.isfinite(got) & np.isfinite(want) & (want != 0)
        rel = np.abs(got[fin] - want[fin]) / np.abs(want[fin])
    bad = np.nonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[0]
    raise AssertionError(f"{what}: {len(bad)} of {2 * w + 1} doubles differ from the restated order, first at {bad[:8].tolist()} "
                         f"(mean [0, {w}), var [{w}, {2 * w}), count {2 * w}); worst relative difference {rel.max() if rel.size else 0:.3e}")


def batch(mode, rows, w, seed):
    """(image x, idx or None) of one call: ``all`` the image itself, ``perm`` a prefix of a permutation of rows + 37, ``repeats``
    drawn with replacement and one pair made equal."""
    g = np.random.default_rng(seed)
    B = rows if mode == "all" else rows + 37
    x = SC.hard_columns(B, seed, w)[0]
    if mode == "all":
        return x, None
    if mode == "perm":
        return x, g.permutation(B)[:rows].astype(np.int64)
    idx = g.integers(0, B, rows).astype(np.int64)
    idx[1] = idx[0]
    return x, idx


# -------------------------------------------------------------------------------------------------------------------- block bits
WIDTHS = (1, 64, 65, 129, 257, 1023)
ROWS = (2, 63, 64, 65, 257)


@pytest.mark.parametrize("mode", ["all", "perm", "repeats"])
@pytest.mark.parametrize("w", WIDTHS)
def test_train_leaves_the_bits_of_the_documented_order(w, mode):
    """Four chained calls from the initial block and from hard_columns' two preloaded blocks; every double of the block after every
    call.  4099 rows (65 chunks) at the two widths whose second column block is ragged."""
    for rows in ROWS + ((4099,) if w in (65, 257) else ()):
        _, b1, b2 = SC.hard_columns(2, 0, w)
        starts = (SC.initial_block(w), b1, b2)
        scs = [_scaler(w, b) for b in starts]
        want = list(starts)
        for call in range(4):
            x, idx = batch(mode, rows, w, 10000 * w + 10 * rows + call)
            xd, idd = dev(x), None if idx is None else dev(idx)
            gathered = x if idx is None else x[idx]
            for s, sc in enumerate(scs):
                sc.train(xd, idd)
                want[s] = SC.ordered_train(want[s], gathered)
                assert_block_bits(block_of(sc), want[s], w, f"w={w} rows={rows} {mode} start={s} call={call}")
            assert want[0][2 * w] == 1 + (call + 1) * rows


# ------------------------------------------------------------------------------------------------------ a bad column stays one
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("rows", [65, 257])
def test_a_non_finite_cell_spoils_its_own_column_only(rows, bad):
    w = 129
    cols = (0, 63, 64, w - 1)
    g = np.random.default_rng(rows)
    clean = (g.standard_normal((rows, w)) * 2.0 + 0.5).astype(np.float32)
    spoiled = clean.copy()
    for j, c in enumerate(cols):
        spoiled[(67 * j + 3) % rows, c] = bad                  # at 257 rows four different chunks, at 65 four rows of the first
    start = SC.hard_columns(2, 1, w)[1]
    want_clean, want = SC.ordered_train(start, clean), SC.ordered_train(start, spoiled)
    sc_clean, sc = _scaler(w, start), _scaler(w, start)
    sc_clean.train(dev(clean))
    sc.train(dev(spoiled))
    got_clean, got = block_of(sc_clean), block_of(sc)
    assert_block_bits(got_clean, want_clean, w, "clean")
    assert_block_bits(got, want, w, "spoiled")                 # NaN-aware: the bad columns too
    other = np.ones(2 * w + 1, bool)
    for c in cols:
        other[c] = other[w + c] = False
        assert not np.isfinite(got[c]) and np.isnan(got[w + c])
    assert np.array_equal(got[other].view(np.int64), want_clean[other].view(np.int64))
    assert np.array_equal(got[other].view(np.int64), got_clean[other].view(np.int64))
    assert np.isfinite(got[other]).all() and got[2 * w] == 1e4 + rows


# -------------------------------------------------------------------------------------------------------------------- gated twin
@pytest.mark.parametrize("use_idx", [False, True])
@pytest.mark.parametrize("w,rows", [(1, 2), (65, 65), (257, 4099)])
def test_gated_train_open_is_the_ungated_call_and_set_touches_nothing(w, rows, use_idx):
    from isaac_rover_orbit_amd import _lib
    x, idx = batch("repeats" if use_idx else "all", rows, w, 31 * w + rows)
    xd, idd = dev(x), None if idx is None else dev(idx)
    start = SC.hard_columns(2, 2, w)[1]
    want = SC.ordered_train(start, x if idx is None else x[idx])
    plain, gated = _scaler(w, start), _scaler(w, start)
    gate = torch.zeros(1, dtype=torch.int32, device=DEV)
    plain.train(xd, idd)
    gated.train(xd, idd, gate=gate)
    assert_block_bits(block_of(gated), want, w, "open gate")
    assert np.array_equal(block_of(gated).view(np.int64), block_of(plain).view(np.int64)) and int(gate) == 0
    # a set gate: the block and a 0x5A-filled workspace keep every byte
    shut = _scaler(w, start)
    shut.ws = torch.full((int(_lib.scaler_workspace_bytes(w, rows)) + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    gate.fill_(1)
    shut.train(xd, idd, gate=gate)
    assert np.array_equal(block_of(shut).view(np.int64), np.asarray(start).view(np.int64))
    assert bool((shut.ws == 0x5A).all()) and int(gate) == 1
    gate.fill_(-7)                                             # any non-zero word
    shut.train(xd, idd, gate=gate)
    assert np.array_equal(block_of(shut).view(np.int64), np.asarray(start).view(np.int64)) and bool((shut.ws == 0x5A).all())


# ----------------------------------------------------------------------------------------------------- transforms on edge blocks
@pytest.mark.parametrize("eps,clip", SC.HPARAMS)
@pytest.mark.parametrize("w", [12, 65, 257])
def test_transforms_on_edge_blocks_have_the_bits_of_the_cpu_oracle(w, eps, clip):
    blk, x = SC.edge_block(w), SC.edge_rows(w)
    rows = x.shape[0]
    sc = _scaler(w, blk, epsilon=eps, clip_threshold=clip)
    xd = dev(x)
    san = SC.numpy_sanitise(x)
    want_f, want_i = SC.numpy_forward(x, blk, w, eps, clip), SC.numpy_inverse(x, blk, w, clip)
    want_fs = SC.numpy_forward(san, blk, w, eps, clip)

    def diff(got, want, what):
        got = got.cpu().numpy()
        if not SC.same_bits32(got, want):
            r, c = np.nonzero((got.view(np.int32) != want.view(np.int32)) & ~(np.isnan(got) & np.isnan(want)))
            cells = [(int(a), int(b), float(x[a, b]), float(blk[b]), float(blk[w + b]), float(got[a, b]), float(want[a, b]))
                     for a, b in list(zip(r, c))[:6]]
            raise AssertionError(f"{what} w={w} eps={eps} clip={clip}: {len(r)} cells differ; (row, col, x, mean, var, got, want): {cells}")

    diff(sc.forward(xd), want_f, "forward")
    diff(sc.inverse(xd), want_i, "inverse")
    raw = torch.full_like(xd, SENTINEL)
    diff(sc.forward(xd, sanitise=True, raw_out=raw), want_fs, "sanitised forward")
    diff(raw, san, "raw_out")
    # rows by idx into an image: the named rows have the oracle's bits, the others keep the sentinel
    idx = np.array([16, 3, 0, 8, 4, 1, 12, 7, 5], np.int64)
    named = np.zeros(rows, bool)
    named[idx] = True
    out, raw = torch.full_like(xd, SENTINEL), torch.full_like(xd, SENTINEL)
    sc.forward(xd, dev(idx), out=out, sanitise=True, raw_out=raw)
    diff(out[dev(named)], want_fs[named], "forward by idx")
    diff(raw[dev(named)], san[named], "raw_out by idx")
    assert bool((out[dev(~named)] == SENTINEL).all()) and bool((raw[dev(~named)] == SENTINEL).all())
    out = torch.full_like(xd, SENTINEL)
    sc.forward(xd, dev(idx), out=out)
    diff(out[dev(named)], want_f[named], "plain forward by idx")
    assert np.array_equal(block_of(sc).view(np.int64), blk.view(np.int64))       # a transform never writes the block


# ------------------------------------------------------------------------------------------ the second pass of the apply kernel
SPAN, ONE_PASS_SPANS = 1024, 8192


def ordinary_block(w, seed):
    g = np.random.default_rng(seed)
    return np.concatenate([g.standard_normal(w) * 1.5, g.random(w) * 4.0 + 0.05, [1e4]])


def spoil(x, g, cells=200):
    """NaN, +inf and -inf at random cells and at both ends, so that sanitise has work in every part of the array."""
    flat = x.reshape(-1)
    at = g.integers(0, flat.size, cells)
    flat[at[0::3]], flat[at[1::3]], flat[at[2::3]] = np.nan, np.inf, -np.inf
    flat[0], flat[-1], flat[-2] = -np.inf, np.nan, np.inf
    return x


def placed(t, off, n):
    """A buffer of n + 8 sentinels, 16-byte aligned, and its view [off, off + n) holding ``t`` (or left as it is)."""
    buf = torch.full((n + 8,), SENTINEL, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + n]
    if t is not None:
        view.copy_(t.reshape(-1))
    return buf, view


def guards_kept(buf, off, n):
    return bool((buf[:off] == SENTINEL).all()) and bool((buf[off + n:] == SENTINEL).all())


def run_apply(sc, kind, x, out, raw):
    if kind == "forward":
        sc.forward(x, out=out)
    elif kind == "inverse":
        sc.inverse(x, out=out)
    else:
        sc.forward(x, out=out, sanitise=True, raw_out=raw)


def oracle(kind, x, blk, w):
    """(out, raw or None) of the CPU oracle for rows x (numpy, (rows, w))."""
    if kind == "forward":
        return SC.numpy_forward(x, blk, w), None
    if kind == "inverse":
        return SC.numpy_inverse(x, blk, w), None
    san = SC.numpy_sanitise(x)
    return SC.numpy_forward(san, blk, w), san


@pytest.mark.parametrize("w,rows", [(965, 8700), (1, 8389700)])
def test_apply_second_pass_without_idx(w, rows):
    """More than 8192 spans of 1024 floats: the workgroups' grid-stride loop repeats and the last span is ragged.  The whole call
    against the same rows cut into two halves of one pass each, bit for bit, and against the CPU oracle on 4096 floats that include
    the first span, the first span of the second pass and the last one."""
    n = rows * w
    n_spans = -(-n // SPAN)
    assert n_spans > ONE_PASS_SPANS and n % SPAN and -(-((rows + 1) // 2 * w) // SPAN) <= ONE_PASS_SPANS
    g = np.random.default_rng(w)
    blk = ordinary_block(w, w)
    x = spoil((g.standard_normal((rows, w)) * 3.0).astype(np.float32), g)
    fixed = np.unique(np.concatenate([np.arange(SPAN), np.arange(ONE_PASS_SPANS * SPAN, min(n, ONE_PASS_SPANS * SPAN + 512)),
                                      np.arange(n - 1536, n)]))
    rest = g.permutation(np.setdiff1d(g.integers(0, n, 3000), fixed))[:4096 - fixed.size]
    sample = np.concatenate([fixed, rest])
    assert sample.size == 4096 and len(np.unique(sample)) == 4096
    cols = sample % w
    blk_s = np.concatenate([blk[cols], blk[w + cols], [blk[2 * w]]])
    sc = _scaler(w, blk)
    half = (rows + 1) // 2 * w
    sample_d = dev(sample)
    for kind in ("forward", "inverse", "sanitise"):
        want, want_raw = oracle(kind, x.reshape(-1)[sample][None, :], blk_s, sample.size)
        for off in (0, 1):
            _, xv = placed(dev(x), off, n)
            bo, out = placed(None, off, n)
            br, raw = placed(None, off, n)
            run_apply(sc, kind, xv.view(rows, w), out.view(rows, w), raw.view(rows, w))
            assert guards_kept(bo, off, n) and guards_kept(br, off, n), (kind, off)
            assert SC.same_bits32(out[sample_d].cpu().numpy(), want[0]), (kind, off)
            if want_raw is not None:
                assert SC.same_bits32(raw[sample_d].cpu().numpy(), want_raw[0]), (kind, off)
            else:
                assert bool((raw == SENTINEL).all())
            # the same rows as two calls of one pass each
            bo2, out2 = placed(None, off, n)
            br2, raw2 = placed(None, off, n)
            for a, b in ((0, half), (half, n)):
                run_apply(sc, kind, xv[a:b].view(-1, w), out2[a:b].view(-1, w), raw2[a:b].view(-1, w))
            assert torch.equal(bo.view(torch.int32), bo2.view(torch.int32)), (kind, off)
            assert torch.equal(br.view(torch.int32), br2.view(torch.int32)), (kind, off)
            del bo, br, bo2, br2, out, raw, out2, raw2, xv


def test_apply_second_pass_with_idx():
    """8200 distinct rows of a 9000-row image at width 5: one wave per row, so rows 8192 ... 8199 of idx belong to the second pass.
    The whole image against the CPU oracle, the rows not named and the floats behind the image keeping their sentinel."""
    w, B, rows = 5, 9000, 8200
    n = B * w
    g = np.random.default_rng(9)
    blk = ordinary_block(w, 9)
    x = spoil((g.standard_normal((B, w)) * 3.0).astype(np.float32), g)
    idx = g.permutation(B)[:rows].astype(np.int64)
    named = np.zeros(B, bool)
    named[idx] = True
    assert named[idx[ONE_PASS_SPANS:]].all() and named.sum() == rows
    sc = _scaler(w, blk)
    idd, named_d = dev(idx), dev(named)
    for kind in ("forward", "inverse", "sanitise"):
        want, want_raw = oracle(kind, x, blk, w)
        for off in (0, 1):
            _, xv = placed(dev(x), off, n)
            outs = []
            for pieces in ((idd,), (idd[:4100].contiguous(), idd[4100:].contiguous())):
                bo, out = placed(None, off, n)
                br, raw = placed(None, off, n)
                for piece in pieces:
                    if kind == "inverse":                      # DeviceScaler.inverse takes no idx: the C ABI's flag through _apply
                        from isaac_rover_orbit_amd import _lib
                        sc._apply(xv.view(B, w), piece, out.view(B, w), _lib.SCALER_INVERSE, None)
                    else:
                        sc.forward(xv.view(B, w), piece, out=out.view(B, w), sanitise=kind == "sanitise",
                                   raw_out=raw.view(B, w) if kind == "sanitise" else None)
                assert guards_kept(bo, off, n) and guards_kept(br, off, n), (kind, off)
                outs.append((bo, br))
                o, r = out.view(B, w), raw.view(B, w)
                assert SC.same_bits32(o[named_d].cpu().numpy(), want[named]), (kind, off, len(pieces))
                assert bool((o[~named_d] == SENTINEL).all()), (kind, off, len(pieces))
                if want_raw is not None:
                    assert SC.same_bits32(r[named_d].cpu().numpy(), want_raw[named]) and bool((r[~named_d] == SENTINEL).all())
                else:
                    assert bool((raw == SENTINEL).all())
            assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
            assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))
