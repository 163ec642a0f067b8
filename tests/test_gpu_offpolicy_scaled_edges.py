"""The staging kernels of the scaled TD3 / SAC path (csrc/offpolicy_scaled_kernels.hip) at widths, phases, blocks and row counts the
feature's own tests leave out:

  * rover_offpolicy_stage_rows at widths below a possible dword head (2, 3), around one 16-byte vector (5, 6, 7) and around the 256
    threads that build the per-column table (255, 256, 257), every destination phase against both source phases, on blocks whose
    (float)var is 0, subnormal, FLT_MAX or inf: bit for bit the fp32 oracle on the CPU and DeviceScaler.forward on the gathered rows
  * more than 2048 rows: the 512 workgroups' loop takes a second pass; a source row out of range reads row 0 and sets the word
  * rover_offpolicy_stage_resolve at action widths 1 and 16 through the C ABI

Every input is made on the CPU and copied to the device."""
import numpy as np
import pytest
import torch

import scaler_cases as SC
from test_gpu_offpolicy_scaled import resolve_numpy

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 777.0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def scaler(w, blk, eps=1e-8, clip=5.0):
    from isaac_rover_orbit_amd.scaler import DeviceScaler
    sc = DeviceScaler(w, DEV, epsilon=eps, clip_threshold=clip)
    sc.block.copy_(torch.from_numpy(blk))
    return sc


def stage(sc, x, src, n, w, x_off=0, o_off=0, bad=None):
    """stage_rows from a ring image ``x_off`` floats past 16-byte alignment into n rows ``o_off`` floats past it; returns the n rows
    after checking that nothing else of the destination buffer, and nothing of the source's, was written."""
    from isaac_rover_orbit_amd import offpolicy_scaled as OS
    R = x.shape[0]
    xbuf = torch.full((R * w + 8,), SENTINEL, device=DEV)
    assert xbuf.data_ptr() % 16 == 0
    xv = xbuf[x_off:x_off + R * w].view(R, w)
    xv.copy_(x)
    keep = xbuf.clone()
    obuf = torch.full(((n + 2) * w + 8,), SENTINEL, device=DEV)
    out = obuf[o_off:o_off + (n + 2) * w].view(n + 2, w)
    OS.stage_rows(sc, xv, src, out[:n], bad)
    assert bool((obuf[:o_off] == SENTINEL).all()) and bool((obuf[o_off + n * w:] == SENTINEL).all()), (w, n, x_off, o_off)
    assert torch.equal(xbuf.view(torch.int32), keep.view(torch.int32))
    return out[:n]


# ------------------------------------------------------------------------------------------------- widths, phases and blocks
@pytest.mark.parametrize("eps,clip", SC.HPARAMS)
@pytest.mark.parametrize("w", [2, 3, 5, 6, 7, 255, 256, 257])
def test_stage_rows_at_small_and_table_edge_widths_on_edge_blocks(w, eps, clip):
    n = 17
    blk, rows = SC.edge_block(w), SC.edge_rows(w)
    src = np.array([(5 * i + 2) % 17 for i in range(n)], np.int64)          # every row of edge_rows once ...
    src[n - 1] = src[0]                                                    # ... but one, and one twice
    want = SC.numpy_forward(rows[src], blk, w, eps, clip)
    sc = scaler(w, blk, eps, clip)
    x, srcd = dev(rows), dev(src)
    fwd = sc.forward(x[srcd].contiguous()).cpu().numpy()
    assert SC.same_bits32(fwd, want)
    for x_off in (0, 1):
        for o_off in (0, 1, 2, 3):
            got = stage(sc, x, srcd, n, w, x_off, o_off).cpu().numpy()
            if not SC.same_bits32(got, want):
                r, c = np.nonzero((got.view(np.int32) != want.view(np.int32)) & ~(np.isnan(got) & np.isnan(want)))
                cells = [(int(a), int(b), float(rows[src[a], b]), float(blk[b]), float(blk[w + b]), float(got[a, b]), float(want[a, b]))
                         for a, b in list(zip(r, c))[:6]]
                raise AssertionError(f"w={w} eps={eps} clip={clip} offsets=({x_off}, {o_off}): {len(r)} cells differ; "
                                     f"(row, col, x, mean, var, got, want): {cells}")
            assert SC.same_bits32(got, fwd)


# ------------------------------------------------------------------------------------------------------------------ second pass
@pytest.mark.parametrize("w,n", [(5, 2048), (5, 2049), (5, 2052), (5, 4100), (965, 4100)])
def test_stage_rows_beyond_2048_rows_takes_a_second_pass(w, n):
    """512 workgroups of four waves hold 2048 rows: at n = 2048 the loop runs once, from 2049 on rows 2048 ... belong to a second
    pass.  Sources drawn with repeats from a 45-row ring, one of them out of range."""
    R = 45
    g = np.random.default_rng(100 * w + n)
    blk = np.concatenate([g.standard_normal(w) * 1.5, g.random(w) * 4.0 + 0.05, [1e4]])
    ring = (g.standard_normal((R, w)) * 3.0).astype(np.float32)
    ring[1, 0], ring[2, w - 1], ring[5, w // 2] = np.nan, np.inf, -np.inf
    src = g.integers(0, R, n).astype(np.int64)
    src[n - 1], src[n - 2], src[0] = 44, 1, 2                  # the last rows of the last pass are known ones
    spoiled = n - 3
    src[spoiled] = R                                           # out of range: row 0's values
    fixed = src.copy()
    fixed[spoiled] = 0
    want = SC.numpy_forward(ring[fixed], blk, w)
    sc = scaler(w, blk)
    x, bad = dev(ring), torch.zeros(1, dtype=torch.int32, device=DEV)
    for x_off, o_off in ((0, 0), (1, 3)):
        bad.zero_()
        got = stage(sc, x, dev(src), n, w, x_off, o_off, bad)
        assert int(bad) == 1
        assert SC.same_bits32(got.cpu().numpy(), want), (x_off, o_off)
        assert torch.equal(got[spoiled].view(torch.int32), sc.forward(x[0:1].contiguous())[0].view(torch.int32))
        assert torch.equal(got.contiguous().view(torch.int32), sc.forward(x[dev(fixed)].contiguous()).view(torch.int32))
    bad.zero_()
    stage(sc, x, dev(fixed), n, w, 0, 0, bad)
    assert int(bad) == 0                                       # ... and a clean call leaves the word alone


# ---------------------------------------------------------------------------------------------------------------------- resolve
@pytest.mark.parametrize("A", [1, 16])
def test_resolve_at_action_widths_1_and_16(A):
    """StagedBatch and stage_resolve hold the action width at the rover's 2, so the call goes through the C ABI; n = 257 (a second
    workgroup of one row), a wrapped ring, repeats, and three bad entries."""
    from isaac_rover_orbit_amd import _fused
    M, N, n = 4, 9, 257
    slots = M + 1
    g = np.random.default_rng(A)
    pos = np.array([4, 0, 2, 3], np.int32)
    act = g.standard_normal((M, N, A)).astype(np.float32)
    act[0, 0, 0], act[1, 2, A - 1] = -0.0, np.nan
    rew = g.standard_normal((M, N)).astype(np.float32)
    rew[0, 1] = -np.inf
    term = g.random((M, N)) < 0.3
    valid = M * N
    idx = g.integers(0, valid, n).astype(np.int64)
    idx[0], idx[256] = 1, 2 * N + 4
    for spoil, pos_used in ((False, pos), (True, np.array([4, 0, slots, 3], np.int32))):
        if spoil:
            idx = idx.copy()
            idx[3], idx[7] = valid, -1
        rows_s, rows_n = (torch.full((n,), -5, dtype=torch.int64, device=DEV) for _ in range(2))
        a_out = torch.full((n * A + 4,), SENTINEL, device=DEV)
        r_out = torch.full((n + 4,), SENTINEL, device=DEV)
        t_out = torch.full((n + 4,), 7, dtype=torch.uint8, device=DEV)
        bad = torch.zeros(1, dtype=torch.int32, device=DEV)
        d = [dev(v) for v in (idx, pos_used, act, rew, term)]
        _fused.launch("rover_offpolicy_stage_resolve", torch.device(DEV, 0), d[0].data_ptr(), n, valid, N, slots, d[1].data_ptr(),
                      d[2].data_ptr(), A, d[3].data_ptr(), d[4].data_ptr(), rows_s.data_ptr(), rows_n.data_ptr(), a_out.data_ptr(),
                      r_out.data_ptr(), t_out.data_ptr(), bad.data_ptr())
        want = resolve_numpy(idx, valid, N, slots, pos_used, act, rew, term)
        assert np.array_equal(rows_s.cpu().numpy(), want[0]) and np.array_equal(rows_n.cpu().numpy(), want[1])
        assert np.array_equal(a_out[:n * A].cpu().numpy().view(np.int32), np.ascontiguousarray(want[2]).reshape(-1).view(np.int32))
        assert np.array_equal(r_out[:n].cpu().numpy().view(np.int32), np.ascontiguousarray(want[3]).view(np.int32))
        assert np.array_equal(t_out[:n].cpu().numpy(), want[4].astype(np.uint8))
        assert bool((a_out[n * A:] == SENTINEL).all()) and bool((r_out[n:] == SENTINEL).all()) and bool((t_out[n:] == 7).all())
        assert int(bad) == int(spoil) == int(want[5])
        assert want[0][0] == 4 * N + 1 and want[1][0] == 1     # memory slot 0: s in the last ring slot, s' in slot 0
        if spoil:
            assert want[0][3] == want[0][7] == 4 * N and want[0][256] == 4 and want[1][256] == N + 4
