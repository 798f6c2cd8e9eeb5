"""GPU test of the tile-major tail of the 256 x 256 tile (mx_gemm_tile.inc, run_tail): a plain bf16 matmul that runs on the
256-row tiles with fp4 weights and at least two slabs of fp8 activations ends its K loop tile by tile and stores the finished tiles
under the last MFMAs.  The grouped launch of the same problem runs the same tile without the tail (write_tile after the loop), so
the two must agree bit for bit: the same MFMAs in the same K order per accumulator, the same rounding chain."""
import pytest

from micromix_amd import mixedgemm

pytestmark = pytest.mark.gpu


def _operands(dev, m, n, k, split, seed, with_bias):
    import torch
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(k, generator=g).to(torch.int16).to(dev)
    w = (torch.randn((n, k), generator=g) * 0.05).to(torch.bfloat16).to(dev)
    x = torch.randn((m, k), generator=g).to(torch.bfloat16).to(dev)
    bias = torch.randn((n,), generator=g).to(torch.bfloat16).to(dev) if with_bias else None
    return mixedgemm.reorder_quantize_x(x, idx, *split), mixedgemm.reorder_quantize_w4(w, idx, *split), bias


@pytest.mark.parametrize("m,n,k,split,with_bias", [
    (4096, 4096, 4096, (0, 0, 4096), False),        # the headline launch
    (4096, 4096, 4096, (0, 0, 4096), True),
    (4000, 3000, 1024, (0, 0, 1024), True),         # tile edges: neither M nor N a multiple of 256
    (3900, 2920, 512, (0, 0, 512), False),
    (4096, 4096, 256, (0, 0, 256), True),           # two slabs: the tail is the whole O segment
    (4096, 4096, 384, (0, 0, 384), False),          # three slabs: one slab-major iteration before the tail
    (4096, 4096, 4096, (2048, 128, 1920), True),    # three segments (rounded in place between them), tail on the last
    (4096, 4096, 4096, (3072, 896, 128), True),     # one O slab: the plain epilogue
])
@pytest.mark.parametrize("rounding", ("reference", "fused"))
def test_tail_equals_plain_epilogue(dev, m, n, k, split, with_bias, rounding):
    import torch
    a, b, bias = _operands(dev, m, n, k, split, m + n + k + split[0], with_bias)
    got = mixedgemm.matmul(a[0], b[0], a[1], b[1], a[2], b[2], a[3], b[3], a[4], b[4], a[5], b[5], bias=bias, split_k=False,
                           rounding=rounding)
    (want,) = mixedgemm.matmul_grouped([a], [b], biases=[bias], rounding=rounding)
    torch.cuda.synchronize()
    assert got.shape == want.shape == (m, n)
    assert torch.equal(got, want), (m, n, k, split, with_bias, rounding, int((got != want).sum()))
