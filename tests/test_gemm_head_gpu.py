"""GPU test of the head of the ping-pong kernel (mx_gemm_tile.inc, run_pingpong): it never zeroes its accumulators -- the first K step
of every accumulator takes the constant 0 as srcC, in the ping-pong loop (count >= 3 slabs) or in the tile-major tail (count = 2) --
and it requests slab 0 before anything else, slab 1 behind a head barrier.  As in test_gemm_pingpong_gpu.py the grouped launch of the
same problem (lock-step loop, zeroed accumulators, write_tile) is the reference, and the two must agree bit for bit; the outputs are
compared as raw int16 so that a NaN equals itself and the sign of a zero counts.

Every case first runs a ping-pong launch on large-magnitude data on the same stream, in the same process: the workgroups of the case
under test then start on accumulator registers that hold large values, and a first K step that accumulated instead of writing would
show up as a difference.

The library gives the 256 x 256 tile to launches that fill the chip, so the small shapes (one tile, 2 x 3 tiles, an edge tile) reach
the ping-pong kernel only under the kernel-developer override MICROMIX_GEMM_TILE=256, which is read once per process: those cases
run in ONE child process (this file as a script)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K2S = (256, 384, 512, 640)          # count = 2, 3, 4, 5 slabs: no period, one period, both parities of the ring
SMALL_SHAPES = ((256, 256), (512, 768), (300, 264))
KINDS = ("random", "nan", "zero")


def _operands(dev, m, n, k, seed, with_bias, kind):
    import torch
    from micromix_amd import mixedgemm
    split = (0, 0, k)
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(k, generator=g).to(torch.int16).to(dev)
    w = (torch.randn((n, k), generator=g) * 0.05).to(torch.bfloat16)
    x = torch.randn((m, k), generator=g).to(torch.bfloat16)
    bias = torch.randn((n,), generator=g).to(torch.bfloat16) if with_bias else None
    if kind == "zero":
        x.zero_()
        w.zero_()
        if bias is not None:
            bias.zero_()
    elif kind == "nan":          # bf16 Inf / NaN in a few activation rows, through the quantizer
        x[1, ::7] = float("inf")
        x[m // 2, 3] = float("nan")
        x[m - 1, ::5] = float("-inf")
    a = mixedgemm.reorder_quantize_x(x.to(dev), idx, *split)
    b = mixedgemm.reorder_quantize_w4(w.to(dev), idx, *split)
    if kind == "nan":            # ... and the e4m3 NaN codes themselves in the quantized rows (e4m3 has no Inf code)
        a[2][2, ::3] = 0x7F
        a[2][m - 2, 1::2] = 0xFF
    return a, b, (bias.to(dev) if bias is not None else None)


def _mm(a, b, bias, rounding):
    from micromix_amd import mixedgemm
    return mixedgemm.matmul(a[0], b[0], a[1], b[1], a[2], b[2], a[3], b[3], a[4], b[4], a[5], b[5], bias=bias, split_k=False,
                            rounding=rounding)


def _is_pingpong(m, n, k):
    from micromix_amd import _lib
    desc = _lib.load().mm_matmul_describe(m, n, 0, 0, k, _lib.MM_W_FP4, 0, 0).decode()
    return "g256" in desc and desc.endswith(", ping-pong K loop"), desc


_dirty = {}


def _dirty_operands(dev, m, n):
    """a ping-pong launch of the case's grid whose accumulators end large (|x| ~ 400, count = 3: loop and tail both run)"""
    import torch
    from micromix_amd import mixedgemm
    if (m, n) not in _dirty:
        g = torch.Generator().manual_seed(99)
        idx = torch.randperm(384, generator=g).to(torch.int16).to(dev)
        x = (torch.randn((m, 384), generator=g) * 400.0).to(torch.bfloat16).to(dev)
        w = (torch.randn((n, 384), generator=g) * 400.0).to(torch.bfloat16).to(dev)
        _dirty[(m, n)] = (mixedgemm.reorder_quantize_x(x, idx, 0, 0, 384), mixedgemm.reorder_quantize_w4(w, idx, 0, 0, 384))
    return _dirty[(m, n)]


def _mismatches(dev, m, n, k, with_bias, rounding, kind):
    """number of output elements whose bits differ between the ping-pong kernel (behind a launch that leaves large accumulators) and
    the grouped launch"""
    import torch
    from micromix_amd import mixedgemm
    a, b, bias = _operands(dev, m, n, k, m + n + k, with_bias, kind)
    da, db = _dirty_operands(dev, m, n)
    (want,) = mixedgemm.matmul_grouped([a], [b], biases=[bias], rounding=rounding)
    big = _mm(da, db, None, rounding)                 # same stream, right in front of the launch under test
    got = _mm(a, b, bias, rounding)
    torch.cuda.synchronize()
    assert float(big.float().abs().nan_to_num().max()) > 1e4     # the launch in front did leave large sums
    assert got.shape == want.shape == (m, n)
    if kind == "nan":
        assert bool(torch.isnan(want.float()).any())
    if kind == "zero":
        assert int(want.view(torch.int16).count_nonzero()) == 0   # +0.0 everywhere, in bits
    return int((got.view(torch.int16) != want.view(torch.int16)).sum())


@pytest.mark.parametrize("rounding", ("reference", "fused"))
@pytest.mark.parametrize("with_bias", (False, True))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", K2S)
def test_head_full_grid(dev, k, kind, with_bias, rounding):
    """256 workgroups, one per CU: the library's own choice of the ping-pong kernel"""
    m = n = 4096
    ok, desc = _is_pingpong(m, n, k)
    assert ok, desc
    assert _mismatches(dev, m, n, k, with_bias, rounding, kind) == 0


def _child():
    import torch
    dev = torch.device("cuda:0")
    out = []
    for m, n in SMALL_SHAPES:
        for k in K2S:
            ok, desc = _is_pingpong(m, n, k)
            if not ok:
                out.append({"case": [m, n, k], "error": desc})
                continue
            for kind in KINDS:
                for with_bias in (False, True):
                    for rounding in ("reference", "fused"):
                        out.append({"case": [m, n, k, kind, with_bias, rounding],
                                    "mismatches": _mismatches(dev, m, n, k, with_bias, rounding, kind)})
    print("HEAD_CASES " + json.dumps(out))


def test_head_small_shapes():
    """one tile, 2 x 3 tiles and an edge tile on the ping-pong kernel (MICROMIX_GEMM_TILE=256), every K, data kind, bias and rounding"""
    env = dict(os.environ, MICROMIX_GEMM_TILE="256")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = next(l for l in r.stdout.splitlines() if l.startswith("HEAD_CASES "))
    cases = json.loads(line[len("HEAD_CASES "):])
    assert len(cases) == len(SMALL_SHAPES) * len(K2S) * len(KINDS) * 4
    bad = [c for c in cases if c.get("mismatches") != 0]
    assert not bad, bad[:10]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    _child()
