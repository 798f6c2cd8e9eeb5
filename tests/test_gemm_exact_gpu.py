"""Exact-answer GPU tests of every GEMM kernel family: inputs whose products and partial sums are exactly representable
(tests/gemm_exact_cases.py; preconditions proved in tests/test_gemm_exact_cpu.py), so that any summation order, any split of K over
waves, workgroups or launches and any tile shape must give the same bits.  Every one of the M x N outputs of every launch is compared
with the closed-form answer for bit equality: no tolerance, no row sample.  The dispatch each case means to reach is asserted through
mm_matmul_describe with the flags the launch uses (the grouped and the device-sized expert launches have no describe entry: their
cases are the row counts of tests/test_grouped_gpu.py and a table that moe_matmul_supported accepts).

Every case carries a seed of its own; `all_cases()` lists (M, N, split, seed, weight modes) of every launch below for the CPU file."""
import numpy as np
import pytest

import gemm_exact_cases as gx
from conftest import bits_from_t, t_from_bits
from micromix_amd import _lib, mixedgemm
from test_matmul_gpu import CHAIN_SPLITS, STREAM_CASES, TILE_KERNELS, _boundary_shapes

pytestmark = pytest.mark.gpu

BOTH = ("w4", "w")
TILE_SPLIT = (256, 128, 256)
PINGPONG = [(4000, 3000, (0, 0, 1024)), (3900, 2920, (0, 0, 512)), (4096, 4096, (0, 0, 256)), (4096, 4096, (0, 0, 384)),
            (4096, 4096, (0, 0, 512))]
CHAIN_MN = (3900, 4090)
WIDE_N, WIDE_M, EDGE_SPLIT = 24608, (1, 8, 16, 17, 32), (128, 128, 128)
EDGE_M = sorted({m for m, n in _boundary_shapes() if n == 264})
EDGE_N = (264, 4104)
SPLIT_K = [(130, 256, (2048, 1024, 1024)), (192, 256, (12288, 1024, 1024)), (128, 1024, (2048, 128, 1920)), (65, 700, (2048, 0, 512))]
# the streaming configurations a grouped / device-sized launch picks by default (tests/test_stream_dispatch_cpu.py asserts that the
# tables below reach every one): 32 features per workgroup once N / 32 x groups fills the CUs -- N = 1024 with eight groups -- per
# tier of the largest group (16 | 32 | 48 | 64 rows); 16 features below, and two ring slots instead of three for two token tiles of
# fp4 weights once K is too long for three (209 slabs)
WIDE_TIERS = [(1024, (256, 128, 256), ms) for ms in ((16, 3, 1, 8, 5, 12, 2, 7), (17, 32, 3, 20, 1, 25, 9, 30), (33, 48, 4, 40, 17, 1, 36, 45),
                                                      (49, 64, 2, 55, 33, 16, 60, 50))]
NARROW_TIERS = [(256, (256, 128, 256), (17, 32, 5)), (256, (256, 128, 256), (33, 48, 2)), (32, (0, 0, 26752), (17,))]
GROUPED = [(256, (256, 128, 128), (3, 0, 17, 64, 1, 40, 8, 33, 5, 12)),                 # ten groups, one empty (tests/test_grouped_gpu.py)
           (512, (128, 0, 128), (128, 200, 65, 512, 300, 96, 1000, 70, 130)),            # nine large groups
           *WIDE_TIERS, *NARROW_TIERS]
GROUPED_IDS = ["ten-groups", "nine-large-groups"] + [f"wide-{16 * t}-rows" for t in (1, 2, 3, 4)] + ["narrow-32-rows", "narrow-48-rows", "two-slots-32-rows"]
MOE = (512, (256, 128, 128), (0, 1, 65, 300))
MOE_TIERS = [*WIDE_TIERS, (256, (256, 128, 256), (16, 0, 7)), *NARROW_TIERS]             # (one more: the device-sized 16-row tier on 16 features)
MOE_TABLES = [MOE, *MOE_TIERS]


def _group_seed(N, split, ms, g):
    """the two tables this file began with keep the seeds they had; every later table's seeds also carry its split and row counts"""
    return _seed(8, N, g) if (N, split, ms) in GROUPED[:2] else _seed(11, N, split, ms, g)


def _seed(*key):
    """a seed per case, a pure function of its shape"""
    s = 17
    for k in key:
        for x in (k if isinstance(k, tuple) else (k,)):
            s = (s * 1000003 + int(x)) % (1 << 31)
    return s


def edge_family(m, n):
    """the kernel a dispatch-edge case means to reach (mx_gemm.hip / plan_tiles at split (128, 128, 128), fp4 weights)"""
    if n == 264:
        return ("mx_gemm_stream_kernel",) if m <= 64 else ("mm::g16::", "(32x64 tiles")
    if m <= 32:
        return ("mx_gemm_stream_kernel",)
    if m <= 64:
        return ("mm::g16::", "(32x64 tiles")
    return ("mm::g32n::", "(64x64 tiles") if m <= 192 else ("mm::g32::", "(64x128 tiles")


def all_cases():
    """(M, N, split, seed, weight modes) of every launch of this file"""
    cases = [(M, N, TILE_SPLIT, _seed(1, M, N), BOTH) for _, _, M, N in TILE_KERNELS]
    cases += [(M, N, split, _seed(2, M, N, split), ("w4",)) for M, N, split in PINGPONG]
    cases += [(*CHAIN_MN, split, _seed(3, split), BOTH) for split in CHAIN_SPLITS]
    cases += [(M, N, split, _seed(4, M, N, split), BOTH) for M, N, split in STREAM_CASES]
    cases += [(M, WIDE_N, EDGE_SPLIT, _seed(5, M), BOTH) for M in WIDE_M]
    cases += [(M, N, EDGE_SPLIT, _seed(6, M, N), ("w4",)) for M in EDGE_M for N in EDGE_N]
    cases += [(M, N, split, _seed(7, M, N, split), BOTH) for M, N, split in SPLIT_K]
    for N, split, ms in GROUPED:
        cases += [(M, N, split, _group_seed(N, split, ms, g), BOTH) for g, M in enumerate(ms)]
    for N, split, ms in MOE_TABLES:
        cases += [(M, N, split, _seed(9, e) if (N, split, ms) == MOE else _seed(10, N, split, ms, e), BOTH) for e, M in enumerate(ms)]
    return cases


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
_last = {}


def case_for(dev, M, N, split, wmode, seed):
    """the case, its intended values and expected outputs shared between the weight modes (the fp64 product runs once, on the GPU)"""
    key = (M, N, tuple(split), seed)
    prev = _last.get("key") == key and _last["case"]
    c = gx.exact_case(M, N, split, wmode, seed, device=dev, values=prev.values if prev else None, want=prev.want if prev else None)
    _last.update(key=key, case=c)
    return c


def to_dev(dev, arrs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs]


def describe(M, N, split, wmode, split_k=False, f32=False):
    """mm_matmul_describe with the flags and the workspace mixedgemm.matmul gives the launch"""
    lib = _lib.load()
    w = _lib.MM_W_FP4 if wmode == "w4" else _lib.MM_W_MATCH
    flags, ws = (_lib.MM_OUT_F32 | _lib.MM_ROUND_ONCE) if f32 else 0, 0
    if split_k and M > 32:
        flags |= _lib.MM_WS_TICKETS_ZEROED | (_lib.MM_SPLIT_K_ALWAYS if split_k == "force" else 0)
        ws = lib.mm_matmul_workspace_bytes(M, N, *split, w, flags)
    return lib.mm_matmul_describe(M, N, *split, w, flags, ws).decode()


def assert_bits(got, want, label):
    """bit equality on every output; on failure the count and the first few (row, col, got, want)"""
    assert got.shape == want.shape and got.dtype == want.dtype, (label, got.shape, want.shape, got.dtype, want.dtype)
    if np.array_equal(got, want):
        return
    g, w = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else (got, want)
    r, c = np.nonzero(g != w)
    first = ", ".join(f"({i}, {j}): got {int(g[i, j]):#x} want {int(w[i, j]):#x}" for i, j in list(zip(r, c))[:6])
    rows, cols = np.unique(r), np.unique(c)
    raise AssertionError(f"{label}: {len(r)} of {got.size} outputs differ, in {len(rows)} rows ({rows[0]}..{rows[-1]}) and {len(cols)} columns "
                         f"({cols[0]}..{cols[-1]}); first: {first}")


def launch(dev, c, **kw):
    import torch
    a, b = to_dev(dev, c.qx), to_dev(dev, c.qw)
    d = mixedgemm.matmul(a[0], b[0], a[1], b[1], a[2], b[2], a[3], b[3], a[4], b[4], a[5], b[5], **kw)
    torch.cuda.synchronize()
    return d.cpu().numpy() if d.dtype == torch.float32 else bits_from_t(d)


def check_launches(dev, c, label, roundings=("reference", "fused"), extras=True, split_k=False):
    """both rounding modes; with `extras` also the bias epilogue (reference rounding) and the fp32 output (the exact sum itself)"""
    import torch
    for rounding in roundings:
        assert_bits(launch(dev, c, rounding=rounding, split_k=split_k), c.want[rounding], f"{label} {rounding}")
    if extras:
        assert_bits(launch(dev, c, bias=t_from_bits(c.bias, dev), split_k=split_k), c.want["reference+bias"], f"{label} reference + bias")
        assert_bits(launch(dev, c, rounding="fused", out_dtype=torch.float32, split_k=split_k), c.want["f32"], f"{label} fp32 output")


# ---- every tile kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wmode", BOTH)
@pytest.mark.parametrize("ns,tile,M,N", TILE_KERNELS, ids=[f"{t[0]}-{t[2]}" for t in TILE_KERNELS])
def test_every_tile_kernel(dev, ns, tile, M, N, wmode):
    for f32 in (False, True):
        desc = describe(M, N, TILE_SPLIT, wmode, f32=f32)
        assert f"mm::{ns}::" in desc and f"({tile} tiles" in desc, desc
    c = case_for(dev, M, N, TILE_SPLIT, wmode, _seed(1, M, N))
    check_launches(dev, c, f"{ns} {M}x{N} {wmode}")


# ---- the 256-row tile: ping-pong K loop and tile-major tail -------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,split", PINGPONG, ids=[f"{m}x{n}x{s[2]}" for m, n, s in PINGPONG])
def test_pingpong_loop_and_tile_major_tail(dev, M, N, split):
    desc = describe(M, N, split, "w4")
    assert "mm::g256::" in desc and desc.endswith(", ping-pong K loop"), desc
    c = case_for(dev, M, N, split, "w4", _seed(2, M, N, split))
    check_launches(dev, c, f"ping-pong {M}x{N} {split}")


# ---- the 256-row tile: chained segment hand-over ------------------------------------------------------------------------------------
@pytest.mark.parametrize("wmode", BOTH)
@pytest.mark.parametrize("split", CHAIN_SPLITS, ids=["_".join(map(str, c)) for c in CHAIN_SPLITS])
def test_chained_segments_on_256_row_tiles(dev, split, wmode):
    M, N = CHAIN_MN
    assert "mm::g256::" in describe(M, N, split, wmode), describe(M, N, split, wmode)
    c = case_for(dev, M, N, split, wmode, _seed(3, split))
    check_launches(dev, c, f"chained {split} {wmode}", extras=split == CHAIN_SPLITS[0])


# ---- skinny and weight-streaming kernels ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wmode", BOTH)
@pytest.mark.parametrize("M,N,split", STREAM_CASES, ids=[f"{c[0]}x{c[1]}-{'_'.join(map(str, c[2]))}" for c in STREAM_CASES])
def test_weight_streaming_kernel(dev, M, N, split, wmode):
    assert "mx_gemm_stream_kernel" in describe(M, N, split, wmode), describe(M, N, split, wmode)
    c = case_for(dev, M, N, split, wmode, _seed(4, M, N, split))
    check_launches(dev, c, f"stream {M}x{N} {split} {wmode}")


@pytest.mark.parametrize("wmode", BOTH)
@pytest.mark.parametrize("M", WIDE_M)
def test_skinny_rows_at_a_wide_n(dev, M, wmode):
    """fused gate + up width: the streaming kernel up to 16 rows, 32 x 64 tiles from 17 on"""
    desc = describe(M, WIDE_N, EDGE_SPLIT, wmode)
    assert ("mx_gemm_stream_kernel" in desc) if M <= 16 else ("mm::g16::" in desc and "(32x64 tiles" in desc), desc
    c = case_for(dev, M, WIDE_N, EDGE_SPLIT, wmode, _seed(5, M))
    check_launches(dev, c, f"wide N {M}x{WIDE_N} {wmode}")


# ---- dispatch edges -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", EDGE_N)
@pytest.mark.parametrize("M", EDGE_M)
def test_dispatch_boundaries(dev, M, N):
    desc = describe(M, N, EDGE_SPLIT, "w4", split_k=True)
    assert all(s in desc for s in edge_family(M, N)), desc
    c = case_for(dev, M, N, EDGE_SPLIT, "w4", _seed(6, M, N))
    check_launches(dev, c, f"boundary {M}x{N}", roundings=("reference",), extras=False, split_k=True)


# ---- split-K: two launches and in-kernel -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wmode", BOTH)
@pytest.mark.parametrize("M,N,split", SPLIT_K, ids=[f"{c[0]}x{c[1]}x{sum(c[2])}" for c in SPLIT_K])
def test_split_k(dev, M, N, split, wmode):
    """forced, default and forbidden: the partial sums are exact, so all three equal the same expected bits"""
    forced, default, off = (describe(M, N, split, wmode, split_k=s) for s in ("force", True, False))
    assert "in-kernel split-K" in forced and "split-K" not in off, (forced, off)
    if sum(split) == 14336:
        assert "split-K" in default and "mm::splitk_reduce_kernel" in default, default          # the two-launch form
    else:
        assert "in-kernel split-K" in default, default
    c = case_for(dev, M, N, split, wmode, _seed(7, M, N, split))
    for split_k in ("force", True, False):
        check_launches(dev, c, f"split-K {M}x{N} {split} {wmode} split_k={split_k}", split_k=split_k)


# ---- grouped launch -----------------------------------------------------------------------------------------------------------------
def _group_cases(N, split, ms, wmode, seeds):
    """one case per group or expert, each with its own seed (products on the host: the groups are small)"""
    return [gx.exact_case(M, N, split, wmode, seed) for M, seed in zip(ms, seeds)]


@pytest.mark.parametrize("wmode", BOTH)
@pytest.mark.parametrize("N,split,ms", GROUPED, ids=GROUPED_IDS)
def test_grouped_launch(dev, N, split, ms, wmode):
    import torch
    cases = _group_cases(N, split, ms, wmode, [_group_seed(N, split, ms, g) for g in range(len(ms))])
    As, Bs = [to_dev(dev, c.qx) for c in cases], [to_dev(dev, c.qw) for c in cases]
    biases = [t_from_bits(c.bias, dev) if g % 2 else None for g, c in enumerate(cases)]
    for rounding in ("reference", "fused"):
        got = mixedgemm.matmul_grouped(As, Bs, biases=biases, rounding=rounding)
        torch.cuda.synchronize()
        assert len(got) == len(ms)
        for g, (y, c) in enumerate(zip(got, cases)):
            assert_bits(bits_from_t(y).reshape(ms[g], N), c.want[rounding + ("+bias" if g % 2 else "")], f"group {g} M={ms[g]} {wmode} {rounding}")


# ---- device-sized expert GEMM -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", (False, True), ids=["plain", "bias"])
@pytest.mark.parametrize("wmode", BOTH)
def test_moe_matmul(dev, wmode, with_bias):
    _moe_matmul(dev, *MOE, wmode, with_bias, [_seed(9, e) for e in range(len(MOE[2]))])


@pytest.mark.parametrize("wmode", BOTH)
@pytest.mark.parametrize("N,split,ms", MOE_TIERS, ids=[f"{n}x{sum(s)}-{max(m)}-rows-{len(m)}-experts" for n, s, m in MOE_TIERS])
def test_moe_matmul_tiers(dev, N, split, ms, wmode):
    """every streaming configuration a device-sized launch picks (the tier from max_rows, the width from N / 32 x experts)"""
    _moe_matmul(dev, N, split, ms, wmode, True, [_seed(10, N, split, ms, e) for e in range(len(ms))])


def _moe_matmul(dev, N, split, ms, wmode, with_bias, seeds):
    import torch
    E, n, K = len(ms), sum(ms), sum(split)
    cases = _group_cases(N, split, ms, wmode, seeds)
    off = np.concatenate([[0], np.cumsum(ms)]).astype(np.int32)
    idx = [torch.arange(K, dtype=torch.int16, device=dev) for _ in ms]           # the packed operands are in reordered order already
    table = mixedgemm.moe_expert_table(idx, [tuple(to_dev(dev, c.qw)) for c in cases], *split,
                                       biases=[t_from_bits(c.bias, dev) for c in cases] if with_bias else None)
    assert mixedgemm.moe_matmul_supported(max(ms), table)
    # the activations of all experts in slot order; expert e's scale bytes at tile off[e] // 128 + e of the packed scale tensors
    A = [np.concatenate([c.qx[i] for c in cases], axis=0) for i in range(3)]
    for i, kseg in enumerate(split):
        sf = np.zeros((mixedgemm.moe_sf_bytes(n, E, kseg),), np.uint8)
        tile = 128 * kseg // 32
        for e, c in enumerate(cases):
            run = c.qx[3 + i][: (ms[e] + 127) // 128 * tile]
            sf[(off[e] // 128 + e) * tile:][: run.size] = run
        A.append(sf)
    A = tuple(to_dev(dev, A))
    offsets = torch.from_numpy(off).to(dev)
    for rounding in ("reference", "fused"):
        D = torch.full((n, N), float("nan"), dtype=torch.bfloat16, device=dev)
        mixedgemm.moe_matmul(A, offsets, table, max(ms), rounding=rounding, out=D)
        torch.cuda.synchronize()
        got = bits_from_t(D)
        for e, c in enumerate(cases):
            assert_bits(got[off[e]:off[e + 1]], c.want[rounding + ("+bias" if with_bias else "")], f"expert {e} ({ms[e]} rows) {wmode} {rounding}")
