"""Which launches take the ping-pong K loop of the 256 x 256 tile (mm_matmul_describe only, no device work): fp4 weights, bf16
output, no split-K, one fp8 x fp4 segment (K[0] = K[1] = 0) of at least two slabs.  Everything else keeps the lock-step loop."""
from micromix_amd import _lib

MARK = ", ping-pong K loop"


def _d(m, n, split, wmode=_lib.MM_W_FP4, flags=0, ws=0):
    return _lib.load().mm_matmul_describe(m, n, *split, wmode, flags, ws).decode()


def test_pingpong_selection():
    head = _d(4096, 4096, (0, 0, 4096))
    assert "g256" in head and "256 workgroups" in head and head.endswith(MARK)
    assert _d(4096, 4096, (0, 0, 256)).endswith(MARK) and _d(4096, 4096, (0, 0, 384)).endswith(MARK)   # two / three O slabs
    assert _d(4000, 3000, (0, 0, 1024)).endswith(MARK)
    tb = _d(4096, 14336, (0, 0, 4096))                 # tail-balanced: the 256-row part
    assert "last 8 tile columns" in tb and tb.endswith(MARK)
    # not covered: mixed splits, one O slab, the "w" mode, fp32 output, split-K, the 128-row tiles
    assert "mm::g256::mx_gemm256_kernel<true,false> x 256" in _d(4096, 4096, (2048, 128, 1920)) and MARK not in _d(4096, 4096, (2048, 128, 1920))
    assert MARK not in _d(4096, 4096, (0, 128, 3968)) and MARK not in _d(4096, 4096, (128, 0, 3968))
    assert MARK not in _d(4096, 4096, (0, 0, 128))
    assert MARK not in _d(4096, 4096, (0, 0, 4096), wmode=_lib.MM_W_MATCH)
    assert MARK not in _d(4096, 4096, (0, 0, 4096), flags=_lib.MM_OUT_F32 | _lib.MM_ROUND_ONCE)
    assert MARK not in _d(192, 256, (0, 0, 4096), flags=_lib.MM_SPLIT_K_ALWAYS, ws=1 << 30)
    assert MARK not in _d(2048, 4096, (0, 0, 4096)) and "g128" in _d(2048, 4096, (0, 0, 4096))
