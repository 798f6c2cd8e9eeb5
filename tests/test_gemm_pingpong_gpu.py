"""GPU test of the ping-pong K loop of the 256 x 256 tile (mx_gemm_tile.inc, run_pingpong): a plain bf16 matmul with fp4 weights whose
K is one fp8 segment of at least two slabs runs its K loop as two wave groups that take turns between MFMAs and LDS / DMA work,
then the tile-major tail.  The grouped launch of the same problem keeps the lock-step loop and write_tile, so the two must agree bit
for bit: every accumulator receives the same MFMAs in the same K order."""
import pytest

from micromix_amd import _lib, mixedgemm

pytestmark = pytest.mark.gpu


def _operands(dev, m, n, k, split, seed, with_bias):
    import torch
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(k, generator=g).to(torch.int16).to(dev)
    w = (torch.randn((n, k), generator=g) * 0.05).to(torch.bfloat16).to(dev)
    x = torch.randn((m, k), generator=g).to(torch.bfloat16).to(dev)
    bias = torch.randn((n,), generator=g).to(torch.bfloat16).to(dev) if with_bias else None
    return mixedgemm.reorder_quantize_x(x, idx, *split), mixedgemm.reorder_quantize_w4(w, idx, *split), bias


@pytest.mark.parametrize("m,n,k,with_bias", [
    (4096, 4096, 4096, False),       # the headline launch
    (4096, 4096, 4096, True),
    (4000, 3000, 1024, True),        # tile edges: neither M nor N a multiple of 256
    (3900, 2920, 512, False),
    (4096, 4096, 256, True),         # two slabs: no ping-pong period, the prologue hands over to the tail
    (4096, 4096, 384, False),        # three slabs: one ping-pong slab
    (4096, 4096, 512, True),         # four slabs
    (4096, 14336, 4096, False),      # tail-balanced launch: the 256-row part runs the ping-pong loop
])
@pytest.mark.parametrize("rounding", ("reference", "fused"))
def test_pingpong_equals_lockstep(dev, m, n, k, with_bias, rounding):
    import torch
    split = (0, 0, k)
    desc = _lib.load().mm_matmul_describe(m, n, *split, _lib.MM_W_FP4, 0, 0).decode()
    assert "g256" in desc and desc.endswith(", ping-pong K loop"), desc
    a, b, bias = _operands(dev, m, n, k, split, m + n + k, with_bias)
    got = mixedgemm.matmul(a[0], b[0], a[1], b[1], a[2], b[2], a[3], b[3], a[4], b[4], a[5], b[5], bias=bias, split_k=False,
                           rounding=rounding)
    (want,) = mixedgemm.matmul_grouped([a], [b], biases=[bias], rounding=rounding)
    torch.cuda.synchronize()
    assert got.shape == want.shape == (m, n)
    assert torch.equal(got, want), (m, n, k, with_bias, rounding, int((got != want).sum()))
