"""mm_rmsnorm_quantize and mm_add_rmsnorm_quantize against the oracle on rows that notice a wrongly ordered sum of squares, on every
kernel behind the two launches and on every way a workgroup walks its rows.  Byte for byte, no tolerance anywhere.

Random rows are nearly blind to rvar (tests/rms_order_cases.py, tests/test_rms_sentinels_cpu.py): the rows here are the sentinels of
tests/golden/rms_sentinels.json -- at least two per wrong order of the sum, and two each for rvar one ulp up and down -- next to
random, all-zero and zeroed-block rows.  A block of R0 distinct rows is repeated down the launch, row r of the launch being row
r % R0 of the block with R0 prime to the grid, so every workgroup meets different rows in every lap, every launched row is compared,
and the oracle runs on R0 rows only.

Row counts per K: 1; R0; 2 CUs + 1, the first count at which K <= 8192 leaves the LDS-DMA ring for the products kernel; and
3 grid + 1 for (an upper bound of) the launch's grid, so every workgroup walks at least three rows -- the prefetching row loops --
and the last lap is ragged.  The residual form runs the same with x = res = s / 2, whose sum is exactly s: the RowAddResidual
instantiations against the oracle itself.  The ring kernel at several rows per workgroup (slot rotation, the counted waits) and the
products kernel at few rows run under the kernel-developer switch MICROMIX_RMS_RING, read once per process: child processes."""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import add_rms_oracle as ar
import rms_order_cases as c
from conftest import t_from_bits
from micromix_amd import mixedgemm
from oracle import mx_oracle as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = sorted(c.SPLITS)
RING_KS = (128, 4224, 8192)


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def grid_bound(k, kind):
    """an upper bound of the grid of the launch (launch_rmsnorm_quantize, launch_add_rmsnorm_quantize): CUs x occupancy, the occupancy
    bounded by what a CU can hold of the launch -- 32 wave slots over the workgroup's waves, 160 KB of LDS over its bytes.
    kind: "staged" -- the products kernel (K <= 8192) or the 16-bit kernel; "ring3" / "ring4" -- the LDS-DMA ring of that depth"""
    kn, ks, ko = c.SPLITS[k]
    t = k // 32
    threads = c.launch_threads(k)
    gpt = 2 if t > 512 else 1
    p = max(64, c.pow2_at_least(t))
    image = ks // 4 * 3 + ko
    if kind == "staged":
        lds = k * (4 if threads <= 256 else 2) + max(p, gpt * threads) * 4 + image
    else:
        assert threads <= 256
        lds = int(kind[-1]) * ((k * 2 + 1023) // 1024 * 1024) + 1024 + max(p, threads) * 4 + image
    return cus() * min(32 // (threads // 64), (160 * 1024) // lds)


def block_size(grid):
    return next(r0 for r0 in (37, 41, 43) if math.gcd(r0, grid) == 1)


@functools.lru_cache(maxsize=None)
def block(k, integer_round, r0):
    """(row bits [r0, K], what each row is, the oracle's packed rows x 3, the oracle's scale bytes [r0, kseg / 32] x 3): computed once
    per (K, integer_round) and shared by every launch of it"""
    fix = c.load_fixture()
    numbers = c.sentinel_rows(fix, k, integer_round)
    assert 4 <= len(numbers) <= r0 - 6
    rows = [c.seeded_row(k, n) for n in numbers]
    what = [sorted(s["order"] for s in fix["sentinels"] if (s["K"], s["integer_round"], s["row"]) == (k, integer_round, n)) for n in numbers]
    idx = c.reorder_index(k).astype(np.int64)
    filler = c.seeded_rows(k, (1 << 31) + int(integer_round), r0 - len(rows))
    filler[0] = 0                                                        # all zero: rvar = 1 / sqrt(eps), every block empty
    filler[1, idx[:32]] = 0                                              # the first group of the first segment empty
    filler[2, idx[k - 64:]] = 0                                          # the last two groups of the last segment empty
    what += [["all zero"], ["zeroed block"], ["zeroed blocks"]] + [["random"]] * (r0 - len(rows) - 3)
    x = np.concatenate([np.stack(rows), filler])
    want = o.rmsnorm_quantize(x, c.norm_weight(k), c.EPS, idx, *c.SPLITS[k], integer_round=integer_round)
    scales = [w[o.sf_valid_offsets(r0, kseg)].reshape(r0, kseg // 32) for w, kseg in zip(want[3:], c.SPLITS[k])]
    return x, what, want[:3], scales


def launch_and_check(dev, k, integer_round, rows, r0, residual):
    import torch
    split = c.SPLITS[k]
    xb, what, packed, scales = block(k, integer_round, r0)
    ridx = torch.arange(rows, device=dev) % r0
    w, tidx = t_from_bits(c.norm_weight(k), dev), torch.from_numpy(c.reorder_index(k)).to(dev)
    x = t_from_bits(xb, dev)[ridx]
    label = f"K={k} rows={rows} integer_round={integer_round} residual={residual}"
    if residual:
        hb = o.f32_to_bf16(o.bf16_to_f32(xb) * np.float32(0.5))
        assert np.array_equal(ar.add_bf16(hb, hb), xb)                   # s / 2 + s / 2 is s exactly
        h = t_from_bits(hb, dev)[ridx]
        s, *got = mixedgemm.add_rmsnorm_quantize_x(h, h.clone(), w, c.EPS, tidx, *split, integer_round=integer_round)
        torch.cuda.synchronize()
        assert torch.equal(s.view(torch.int16), x.view(torch.int16)), f"{label}: the sum is not the row"
    else:
        got = mixedgemm.rmsnorm_quantize_x(x, w, c.EPS, tidx, *split, integer_round=integer_round)
        torch.cuda.synchronize()
    bad = torch.zeros(rows, dtype=torch.bool, device=dev)
    for i, kseg in enumerate(split):
        if not kseg:
            continue
        want = torch.from_numpy(np.ascontiguousarray(packed[i])).to(dev)[ridx]
        assert got[i].shape == want.shape, (label, i)
        bad |= (got[i] != want).any(dim=1)
        r, j = np.arange(rows)[:, None], np.arange(kseg // 32)[None, :]
        offs = torch.from_numpy(o.sf_offset(r, j, kseg)).to(dev)
        bad |= (got[3 + i][offs] != torch.from_numpy(scales[i]).to(dev)[ridx]).any(dim=1)
    if bool(bad.any()):
        where = torch.nonzero(bad).flatten().cpu().numpy()
        kinds = sorted({n for r in set((where % r0).tolist()) for n in what[r]})
        raise AssertionError(f"{label}: {len(where)} rows differ from the oracle (first {where[:8].tolist()}); they are the rows that notice {kinds}")


def row_counts(k, r0, kind="staged"):
    return (1, r0, 2 * cus() + 1, 3 * grid_bound(k, kind) + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("residual", (False, True), ids=("plain", "add"))
@pytest.mark.parametrize("integer_round", (True, False))
@pytest.mark.parametrize("k", KS)
def test_every_kernel_and_row_walk_matches_the_oracle(dev, k, integer_round, residual):
    grid = grid_bound(k, "staged")
    r0 = block_size(grid)
    assert math.gcd(r0, grid) == 1 and math.gcd(r0, cus()) == 1
    for rows in row_counts(k, r0):
        launch_and_check(dev, k, integer_round, rows, r0, residual)


@pytest.mark.gpu
def test_largest_launch_is_three_laps_of_one_workgroup_per_cu(dev):
    assert row_counts(32768, 37)[-1] == 3 * cus() + 1          # 769 rows of K = 32768 with 256 CUs


CHILD = r'''
import sys
import torch
sys.path.insert(0, "tests")
from conftest import *            # noqa: F401,F403  (sys.path set-up)
import test_rms_order_gpu as t
dev = torch.device("cuda:0")
ring = int(sys.argv[1])
n = 0
for k in t.RING_KS:
    for integer_round in (True, False):
        if ring:
            grid = t.grid_bound(k, "ring%d" % ring)
            r0 = t.block_size(grid)
            rows = 3 * grid + 1               # several rows per workgroup: the slots rotate, both counted waits run, the last lap is ragged
        else:
            r0 = rows = t.block_size(t.grid_bound(k, "staged"))     # the products kernel where the launcher would choose the ring
        t.launch_and_check(dev, k, integer_round, rows, r0, False)
        n += 1
print("ok", n)
'''


@pytest.mark.gpu
@pytest.mark.parametrize("ring", (3, 4, 0))
def test_pinned_ring_depths_and_the_products_kernel_at_few_rows(ring):
    env = dict(os.environ, MICROMIX_RMS_RING=str(ring), PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", CHILD, str(ring)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"ok {2 * len(RING_KS)}" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
