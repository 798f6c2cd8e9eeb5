"""mixedgemm.moe_matmul against matmul_grouped at a shape where the streaming kernels' configuration matters ("Which
bits"): K = 1024 -- eight slabs, so the waves of a workgroup sum more than one slab each and the number of waves NW that share K sets
the order of the fp32 partial sums -- and N = 2048, wide enough for four groups to fill the CUs (the `wide` configurations, 32 features
per workgroup; NW = 4 above the 16-row tier).  The shapes of tests/test_moe_device_sized_gpu.py have K <= 512 and N <= 512: every
configuration gives the same bits there, and only the 64 x 64 tile is launched.

What the library states, and what is asserted here bit for bit:
  * an expert's rows carry the bits mm_matmul_grouped gives them in a launch that splits K over the same number of waves: NW = 4 when
    the launch is wide and its tier is above 16 rows, 8 otherwise.  The device-sized launch takes the tier from max_rows and counts
    min(E, n, 8) groups; mm_matmul_grouped takes the tier from the largest group of at most 64 rows and counts those groups.  The tier
    itself (token tiles), the features per workgroup and the ring depth change no bit;
  * where the two differ in NW the device-sized result is the one mm_matmul_grouped gives the same rows inside a launch of that NW;
  * experts above 64 rows are on the tiled kernels in both, whose tile size changes no bit: the 128 x 128, 128 x 256 and 256 x 256
    tiles of the device-sized launch, chosen from its host bound on the tiles, against whatever mm_matmul_grouped picks."""
import numpy as np
import pytest

from conftest import bits_from_t, t_from_bits
from micromix_amd import mixedgemm
from model_case import gen_bf16, gen_index
from oracle import mx_oracle as o

pytestmark = pytest.mark.gpu
PACKED = ("BN", "BS", "BO", "SFBN", "SFBS", "SFBO")
E, N, SPLIT = 8, 2048, (512, 256, 256)
K = sum(SPLIT)


@pytest.fixture(scope="module")
def experts(dev):
    """eight experts' quantized weights [N, K] (fp4 weights, the Mixtral mode) with reorder indices of their own, and their device table"""
    import torch
    from micromix_amd.qlinear import QLinearLayer
    rng = np.random.default_rng(2048)
    layers = []
    for e in range(E):
        lin = torch.nn.Linear(K, N, bias=False, dtype=torch.bfloat16, device=dev)
        lin.weight.data = t_from_bits(o.f32_to_bf16((0.05 * rng.standard_normal((N, K))).astype(np.float32)), dev)
        idx = gen_index(dev, K, 77 + e)
        layers.append(QLinearLayer(lin, p8_num=SPLIT[2], p6_num=SPLIT[1], reorder_index=idx, weight_mode="w4", rounding="reference"))
    idx = [l.reorder_index for l in layers]
    B = [tuple(getattr(l, n) for n in PACKED) for l in layers]
    return idx, B, mixedgemm.moe_expert_table(idx, B, *SPLIT)


def cus(dev):
    import torch
    return torch.cuda.get_device_properties(dev).multi_processor_count


def waves(tier_rows, groups, dev):
    """NW of the streaming configuration for a launch of `groups` groups whose tier is that of tier_rows (mx_gemm_stream.hip)"""
    wide = (N + 31) // 32 * groups >= cus(dev)
    return 4 if wide and tier_rows > 16 else 8


def host_waves(counts, dev):
    small = [c for c in counts if 0 < c <= 64]
    assert len(small) <= 8                                    # one launch of mm_matmul_grouped
    return waves(max(small), len(small), dev)


def device_waves(counts, max_rows, dev):
    return waves(min(max_rows, 64), min(E, sum(counts), 8), dev)


def run_both(dev, experts, counts, max_rows, rounding, rows):
    """(bits of moe_matmul with D pre-filled with NaN, bits of matmul_grouped(outs=), offsets) on the first sum(counts) rows of `rows`"""
    import torch
    idx, B, table = experts
    off = np.concatenate([[0], np.cumsum(counts)]).tolist()
    n = off[-1]
    offsets = torch.tensor(off, dtype=torch.int32, device=dev)
    x = rows[:n]
    q = mixedgemm.moe_quantize(x, None, offsets, table)
    qe = mixedgemm.reorder_quantize_x_grouped([x[off[e]:off[e + 1]] for e in range(E)], idx, *SPLIT)
    want = torch.zeros((n, N), dtype=torch.bfloat16, device=dev)
    mixedgemm.matmul_grouped(qe, B, rounding=rounding, outs=[want[off[e]:off[e + 1]] for e in range(E)])
    D = torch.full((n, N), float("nan"), dtype=torch.bfloat16, device=dev)
    mixedgemm.moe_matmul(q, offsets, table, max_rows, rounding=rounding, out=D)
    torch.cuda.synchronize()
    return bits_from_t(D), bits_from_t(want), off


@pytest.fixture(scope="module")
def rows(dev):
    return gen_bf16(dev, 3300, K, 4242, "x")


# (rows per expert, max_rows): the two launches split K over the same number of waves, through different configurations
SAME_WAVES = {
    # max_rows in a higher tier than the largest group: <2, 2, 2, 4> against <2, 4, 2, 4> and <2, 3, 2, 4>
    "largest 20, max_rows 64": ((20,) * 8, 64),
    "largest 20, max_rows 48": ((20, 17, 3, 0, 20, 1, 9, 0), 48),
    # ... inside the 16-row tier of both: the same configuration
    "largest 16, max_rows 16": ((9, 1, 0, 16, 3, 0, 0, 7), 16),
    # fewer groups with rows than min(E, n, 8): one group is not wide on the host, <1, 1, 3, 8>, against <2, 1, 2, 8>
    "one group of 12": ((0, 0, 12, 0, 0, 0, 0, 0), 12),
    "two groups, largest 16": ((0, 16, 0, 0, 0, 5, 0, 0), 16),
    # groups on the tiled kernels beside them: 128 x 128, 128 x 256 and 256 x 256 tiles from the host bound (n = 600, 1 500, 3 300)
    "n 600": ((64, 65, 130, 260, 20, 3, 9, 49), 600),
    "n 1500": ((64, 500, 40, 700, 33, 91, 8, 64), 1500),
    "n 3300": ((1500, 64, 50, 900, 17, 5, 700, 64), 3300),
}


@pytest.mark.parametrize("name", list(SAME_WAVES))
def test_moe_matmul_is_matmul_grouped_bit_for_bit_at_equal_waves(dev, experts, rows, name):
    counts, max_rows = SAME_WAVES[name]
    assert host_waves(counts, dev) == device_waves(counts, max_rows, dev), "the case is not what its name says on this device"
    for rounding in ("reference", "fused"):
        got, want, off = run_both(dev, experts, counts, max_rows, rounding, rows)
        assert not np.isnan(o.bf16_to_f32(got)).any(), f"{name} {rounding}: unwritten rows"
        for e in range(E):
            assert np.array_equal(got[off[e]:off[e + 1]], want[off[e]:off[e + 1]]), f"{name} {rounding}: expert {e} ({counts[e]} rows) differs"


# (rows per expert, max_rows, rows per expert of the host launch that splits K like the device-sized one): the experts named in
# `same` hold the same rows in both routings -- the leading experts, so their offsets agree
OTHER_WAVES = {
    # max_rows in the 32-row tier, every group in the 16-row tier: the host runs NW = 8, the device-sized launch NW = 4 -- the bits of
    # the same rows in a host launch whose largest group is above 16
    "largest 16, max_rows 32": ((16, 9, 4, 16, 1, 1, 1, 1), 32, (16, 9, 4, 16, 20, 1, 1, 1), (0, 1, 2, 3)),
    # one group with rows, above the 16-row tier: not wide on the host (NW = 8), wide here (NW = 4) -- the bits of a full host launch
    "one group of 20": ((20, 0, 0, 0, 0, 0, 0, 0), 20, (20,) * 8, (0,)),
}


@pytest.mark.parametrize("name", list(OTHER_WAVES))
def test_moe_matmul_at_other_waves_is_the_grouped_launch_of_those_waves(dev, experts, rows, name):
    counts, max_rows, host_counts, same = OTHER_WAVES[name]
    assert host_waves(counts, dev) == 8 and device_waves(counts, max_rows, dev) == 4 and host_waves(host_counts, dev) == 4, \
        "the case is not what its name says on this device"
    for rounding in ("reference", "fused"):
        got, own_want, off = run_both(dev, experts, counts, max_rows, rounding, rows)
        _, want, host_off = run_both(dev, experts, host_counts, 64, rounding, rows)
        assert not np.isnan(o.bf16_to_f32(got)).any(), f"{name} {rounding}: unwritten rows"
        for e in same:
            assert off[e] == host_off[e] and counts[e] == host_counts[e]
            assert np.array_equal(got[off[e]:off[e + 1]], want[host_off[e]:host_off[e + 1]]), \
                f"{name} {rounding}: expert {e} ({counts[e]} rows) differs from the grouped launch on four waves"
        print(f"{name} {rounding}: {int((got != own_want).sum())} of {got.size} outputs differ from the grouped launch on eight waves")
