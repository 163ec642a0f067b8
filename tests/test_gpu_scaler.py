"""The width-generic running scaler on the MI355X (include/rover_scaler.h, isaac_rover_orbit_amd.scaler.DeviceScaler): statistics
against float64 numpy at the lift test's bounds, the transforms bit for bit against the torch expression on the same block,
placement with idx, aliasing, ragged vector tails and misaligned bases, stale workspaces and run-to-run bits."""
import numpy as np
import pytest
import torch

from lift_ppo_reference import NumpyScaler

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLT_MAX = float(np.finfo(np.float32).max)
WIDTHS = (1, 63, 64, 965, 1024)
# 2: the least torch.var accepts; 63 / 64 / 65: one chunk of 64 rows, ragged and full, and the first row of a second one;
# 255 / 256 / 257 and 4099: several chunks with a ragged last one
ROWS = (2, 63, 64, 65, 255, 256, 257, 4099)


def _scaler(w, **kw):
    from isaac_rover_orbit_amd.scaler import DeviceScaler
    return DeviceScaler(w, DEV, **kw)


def _biteq(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _fwd_expr(x, blk, w, eps=1e-8, clip=5.0):
    mean, var = blk[:w], blk[w:2 * w]
    return torch.clamp((x - mean.float()) / (torch.sqrt(var.float()) + eps), min=-clip, max=clip)


def _inv_expr(x, blk, w, clip=5.0):
    mean, var = blk[:w], blk[w:2 * w]
    return torch.sqrt(var.float()) * torch.clamp(x, min=-clip, max=clip) + mean.float()


@pytest.mark.parametrize("mode", ["all", "perm", "repeats"])
@pytest.mark.parametrize("w", WIDTHS)
def test_statistics_match_float64_numpy(w, mode):
    """Four chained updates on data of differing scale and offset; mean / variance at rtol 1e-12 (atol 1e-12 on the mean), the
    count exact -- the bounds of tests/test_gpu_lift_ppo.py for the one-workgroup-per-column scaler."""
    g = torch.Generator(device=DEV).manual_seed(1000 * w + len(mode))
    for rows in ROWS:
        sc, ns = _scaler(w), NumpyScaler(w)
        for i in range(4):
            B = rows if mode == "all" else rows + 37
            x = (torch.randn(B, w, device=DEV, generator=g) * (1 + 3 * i) + i).contiguous()
            if mode == "all":
                idx = None
            elif mode == "perm":
                idx = torch.randperm(B, device=DEV, generator=g)[:rows].contiguous()
            else:
                idx = torch.randint(0, B, (rows,), device=DEV, generator=g)
                idx[1] = idx[0]
            sc.train(x, idx)
            ns.train((x if idx is None else x[idx]).double().cpu().numpy())
            blk = sc.block.cpu().numpy()
            np.testing.assert_allclose(blk[:w], ns.mean, rtol=1e-12, atol=1e-12, err_msg=f"mean rows={rows} call={i}")
            np.testing.assert_allclose(blk[w:2 * w], ns.var, rtol=1e-12, err_msg=f"var rows={rows} call={i}")
            assert blk[2 * w] == ns.count == 1 + (i + 1) * rows


@pytest.mark.parametrize("w", WIDTHS)
def test_forward_and_inverse_have_the_bits_of_the_torch_expression(w):
    g = torch.Generator(device=DEV).manual_seed(w)
    sc = _scaler(w)
    for i in range(2):
        rows = 257 + 70 * i
        x = (torch.randn(rows, w, device=DEV, generator=g) * (1 + 3 * i) + i).contiguous()
        x[0, 0], x[1, w - 1] = 1e4, -1e4                                            # beyond the clamp
        sc.train(x)
        out = sc.forward(x)
        assert _biteq(out, _fwd_expr(x, sc.block, w))
        assert float(out.max()) == 5.0 and float(out.min()) == -5.0
        y = (torch.randn(333, w, device=DEV, generator=g) * 4).contiguous()
        y[0, 0], y[1, 0] = 77.0, -77.0                                              # beyond the clamp
        assert _biteq(sc.inverse(y), _inv_expr(y, sc.block, w))
    # NaN passes both clamps, as torch.clamp has it
    x[2, 0] = float("nan")
    for got, want in ((sc.forward(x), _fwd_expr(x, sc.block, w)), (sc.inverse(x), _inv_expr(x, sc.block, w))):
        assert bool(got[2, 0].isnan()) and torch.equal(got.isnan(), want.isnan())
        assert _biteq(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0))
    # other hyper-parameters
    sc2 = _scaler(w, epsilon=1e-3, clip_threshold=1.5)
    sc2.block.copy_(sc.block)
    x[2, 0] = 0.25
    assert _biteq(sc2.forward(x), _fwd_expr(x, sc.block, w, 1e-3, 1.5)) and _biteq(sc2.inverse(x), _inv_expr(x, sc.block, w, 1.5))


@pytest.mark.parametrize("w,rows", [(965, 19), (64, 300), (1, 1027)])
def test_sanitise_has_the_bits_of_nan_to_num(w, rows):
    g = torch.Generator(device=DEV).manual_seed(7)
    sc = _scaler(w)
    sc.train((torch.randn(500, w, device=DEV, generator=g) * 2 + 1).contiguous())
    x = (torch.randn(rows, w, device=DEV, generator=g) * 3).contiguous()
    flat = x.view(-1)
    cells = torch.randperm(flat.numel(), device=DEV, generator=g)[:min(90, flat.numel() // 2)]
    flat[cells[0::3]], flat[cells[1::3]], flat[cells[2::3]] = float("nan"), float("inf"), float("-inf")
    flat[0], flat[-1] = float("-inf"), float("nan")
    want = torch.nan_to_num(x, nan=0.0, posinf=FLT_MAX, neginf=0.0)
    raw = torch.full_like(x, 777.0)
    out = sc.forward(x, sanitise=True, raw_out=raw)
    assert _biteq(raw, want) and _biteq(out, _fwd_expr(want, sc.block, w)) and torch.isfinite(out).all()
    assert _biteq(sc.forward(x, sanitise=True), out)                                  # without the raw copy
    assert not torch.isfinite(sc.forward(x)).all()                                    # ... and the flag is what does it
    keep = x.clone()
    assert _biteq(sc.forward(x, out=x, sanitise=True), out) and not _biteq(x, keep)   # in place


def test_a_constant_column_stays_finite():
    w = 5
    sc, ns = _scaler(w), NumpyScaler(w)
    g = torch.Generator(device=DEV).manual_seed(3)
    for i in range(4):
        x = torch.randn(300 + i, w, device=DEV, generator=g)
        x[:, 1], x[:, 3] = 2.5, 0.0
        sc.train(x.contiguous())
        ns.train(x.double().cpu().numpy())
        out = sc.forward(x.contiguous())
        assert torch.isfinite(sc.block).all() and torch.isfinite(out).all() and _biteq(out, _fwd_expr(x, sc.block, w))
    blk = sc.block.cpu().numpy()
    assert (blk[w:2 * w] > 0).all()
    np.testing.assert_allclose(blk[:w], ns.mean, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(blk[w:2 * w], ns.var, rtol=1e-12)


@pytest.mark.parametrize("w,B,rows", [(965, 40, 13), (63, 300, 257), (1, 100, 33), (1024, 9, 4)])
def test_idx_writes_the_named_rows_in_place_and_no_others(w, B, rows):
    g = torch.Generator(device=DEV).manual_seed(11)
    sc = _scaler(w)
    x = (torch.randn(B, w, device=DEV, generator=g) * 2 + 0.5).contiguous()
    x[3, 0] = float("-inf")
    sc.train(x, torch.arange(4, B, device=DEV))
    perm = torch.randperm(B, device=DEV, generator=g)
    idx = torch.cat([torch.tensor([3], device=DEV), perm[perm != 3][:rows - 1]]).contiguous()      # distinct, the -inf row among them
    named = torch.zeros(B, dtype=torch.bool, device=DEV)
    named[idx] = True
    full = sc.forward(x, sanitise=True)
    out = torch.full_like(x, -123.25)
    raw = torch.full_like(x, 55.5)
    sc.forward(x, idx, out=out, sanitise=True, raw_out=raw)
    assert _biteq(out[named], full[named]) and bool((out[~named] == -123.25).all())
    assert _biteq(raw[named], torch.nan_to_num(x, nan=0.0, posinf=FLT_MAX, neginf=0.0)[named]) and bool((raw[~named] == 55.5).all())
    # repeats write the same value twice
    rep = torch.cat([idx, idx[:2]]).contiguous()
    out2 = torch.full_like(x, -123.25)
    sc.forward(x, rep, out=out2, sanitise=True)
    assert _biteq(out2, out)
    # in place within the image itself
    img = x.clone()
    sc.forward(img, idx, out=img, sanitise=True)
    assert _biteq(img[named], full[named]) and _biteq(img[~named], x[~named])


@pytest.mark.parametrize("w,rows", [(965, 7), (965, 1), (63, 65), (64, 17), (1, 1027), (1, 3), (1024, 3), (5, 410)])
def test_ragged_tails_and_misaligned_bases_give_the_same_bits(w, rows):
    """A base 4 bytes past 16-byte alignment moves every vector boundary; x, out and raw_out offset alike take the vector path
    with a scalar head, offset differently the scalar path.  All give the aligned call's bits."""
    g = torch.Generator(device=DEV).manual_seed(13)
    sc = _scaler(w)
    sc.train((torch.randn(64, w, device=DEV, generator=g) * 2 - 1).contiguous())
    n = rows * w
    x0 = (torch.randn(rows, w, device=DEV, generator=g) * 3).contiguous()
    x0[0, 0] = float("-inf")
    want_raw = torch.nan_to_num(x0, nan=0.0, posinf=FLT_MAX, neginf=0.0)
    want, want_inv = _fwd_expr(want_raw, sc.block, w), _inv_expr(want_raw, sc.block, w)

    def place(t, off):
        buf = torch.full((n + 8,), 999.0, device=DEV)
        assert buf.data_ptr() % 16 == 0
        view = buf[off:off + n].view(rows, w)
        if t is not None:
            view.copy_(t)
        return buf, view

    for ox, oo, orr in ((0, 0, 0), (1, 1, 1), (3, 3, 3), (1, 0, 0), (0, 2, 0), (0, 0, 3), (1, 1, None), (2, 1, None)):
        _, x = place(x0, ox)
        bo, out = place(None, oo)
        br, raw = place(None, orr) if orr is not None else (None, None)
        sc.forward(x, out=out, sanitise=True, raw_out=raw)
        assert _biteq(out, want), (ox, oo, orr)
        assert bool((bo[:oo] == 999.0).all()) and bool((bo[oo + n:] == 999.0).all())   # nothing outside the rows
        if raw is not None:
            assert _biteq(raw, want_raw) and bool((br[:orr] == 999.0).all()) and bool((br[orr + n:] == 999.0).all())
        _, xi = place(want_raw, ox)
        bo, out = place(None, oo)
        sc.inverse(xi, out=out)
        assert _biteq(out, want_inv) and bool((bo[:oo] == 999.0).all()) and bool((bo[oo + n:] == 999.0).all())
    # rows named by idx in a misaligned image: each row has an alignment of its own at an odd width
    idx = torch.arange(rows - 1, -1, -2, device=DEV).contiguous()
    _, x = place(x0, 1)
    bo, out = place(None, 1)
    sc.forward(x, idx, out=out, sanitise=True)
    assert _biteq(out[idx], want[idx])


@pytest.mark.parametrize("w,rows", [(965, 4099), (1, 257), (64, 64)])
def test_stale_workspace_and_repeated_calls_give_the_same_block_bits(w, rows):
    from isaac_rover_orbit_amd import _lib
    g = torch.Generator(device=DEV).manual_seed(17)
    x = (torch.randn(rows, w, device=DEV, generator=g) * 5 + 2).contiguous()
    idx = torch.randint(0, rows, (rows,), device=DEV, generator=g)
    blocks = []
    for fill in (None, 0xFF, 0x00, None):
        for use_idx in (False, True):
            sc = _scaler(w)
            if fill is not None:
                sc.ws = torch.full((_lib.scaler_workspace_bytes(w, rows) + 64,), fill, dtype=torch.uint8, device=DEV)
            sc.train(x, idx if use_idx else None)
            sc.train(x, idx if use_idx else None)                                  # the second call reads the first one's leftovers
            blocks.append((use_idx, sc.block.clone()))
    torch.cuda.synchronize()
    for use_idx, blk in blocks:
        ref = next(b for u, b in blocks if u == use_idx)
        assert torch.equal(blk.view(torch.int64), ref.view(torch.int64))
    assert not torch.equal(blocks[0][1], blocks[1][1])


def test_state_dict_round_trips_with_skrl_keys():
    from isaac_rover_orbit_amd.lift_ppo import RunningStandardScaler
    sc = _scaler(965)
    x = torch.randn(100, 965, device=DEV).contiguous()
    sc.train(x)
    sd = sc.state_dict()
    assert set(sd) == {"running_mean", "running_variance", "current_count"} and float(sd["current_count"]) == 101.0
    ts = RunningStandardScaler(965, device=DEV)
    ts.load_state_dict(sd)
    assert _biteq(ts(x), sc.forward(x))
    back = _scaler(965)
    back.load_state_dict(ts.state_dict())
    assert torch.equal(back.block, sc.block)
    with pytest.raises(ValueError):
        _scaler(1).load_state_dict(sd)
    with pytest.raises(ValueError):
        _scaler(1025)
