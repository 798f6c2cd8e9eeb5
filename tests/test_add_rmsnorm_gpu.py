"""GPU tests of the residual add fused into the RMSNorm quantizer (mm_add_rmsnorm_quantize, mixedgemm.add_rmsnorm_quantize_x) and of
`residual=` through QLinearLayer / FusedQLinear / FusedMLP.  No tolerance anywhere: S_out is bit-equal to the numpy rule of
tests/add_rms_oracle.py, the six buffers are byte for byte mm_rmsnorm_quantize of S_out, and a chain of layers that threads the
residual is bit-equal to the same chain with torch adds."""
import os
import subprocess
import sys

import numpy as np
import pytest

import add_rms_oracle as ar
from conftest import bits_from_t, t_from_bits
from micromix_amd import _lib, mixedgemm
from micromix_amd.qlinear import FusedMLP, FusedQLinear, QLinearLayer
from oracle import mx_oracle as o

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-5

# (K, split): the smallest shapes that reach each code path of the two staging kernels
SHAPES = {128: (0, 128, 0),                 # four group threads, the zero-padded tree
          384: (128, 128, 128),             # all three segments and the code image
          4096: (2048, 128, 1920),          # the products kernel
          8192: (4096, 2048, 2048),         # ... and its limit
          8320: (4096, 128, 4096),          # the 16-bit kernel at one group per thread
          16512: (8192, 128, 8192)}         # two groups per thread


def many_rows(K):
    """3 x grid + 1 rows for a grid of CUs x occupancy workgroups (launch_add_rmsnorm_quantize): every workgroup walks at least three
    rows and the prefetch runs.  The occupancy is bounded from above by what the hardware can hold of this launch -- 32 wave slots per
    CU over the workgroup's waves, 160 KB of LDS over its bytes -- so the real grid is at most this one."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    kn, ks, ko = SHAPES[K]
    threads = (K // 32 + 63) // 64 * 64
    lds = K * 4 + max(threads, 64) * 4 + ks // 4 * 3 + ko
    return 3 * cus * min(32 // (threads // 64), (160 * 1024) // lds) + 1


def inputs(rows, K, seed):
    """x, r bit patterns: gaussian rows; row 1 (if any) x = -r; row 2 (if any) carries +-inf, NaN and inf - inf; row 0 subnormal sums"""
    rng = np.random.default_rng(seed)
    x = o.f32_to_bf16(rng.standard_normal((rows, K)).astype(np.float32))
    r = o.f32_to_bf16((2 * rng.standard_normal((rows, K))).astype(np.float32))
    x[0, :8] = [0x0001, 0x0040, 0x807F, 0x0001, 0x0000, 0x8000, 0x0033, 0x8001]     # subnormals whose sums stay subnormal (or reach the
    r[0, :8] = [0x0001, 0x0040, 0x8001, 0x8002, 0x0003, 0x0001, 0x0011, 0x8001]     # smallest normal)
    if rows > 1:
        r[1] = x[1] ^ 0x8000
    if rows > 2:
        x[2, :6] = [0x7F80, 0xFF80, 0x7F80, 0x7FC1, 0x7F7F, 0x3F80]
        r[2, :6] = [0x3F80, 0x3F80, 0xFF80, 0x0000, 0x7F7F, 0xFF80]
    w = o.f32_to_bf16((1.0 + 0.2 * rng.standard_normal(K)).astype(np.float32))
    idx = rng.permutation(K).astype(np.int16)                                        # a reorder index of its own per call
    return x, r, w, idx


def buffers(alloc_rows, K, split, dev):
    """S_out and the six outputs for alloc_rows rows, every byte 0xFF"""
    import torch
    kn, ks, ko = split
    sizes = [alloc_rows * K * 2, alloc_rows * (kn // 2), alloc_rows * (ks // 4 * 3), alloc_rows * ko] + [mixedgemm._sf_bytes_x(alloc_rows, s) for s in split]
    return [torch.full((max(n, 16),), 0xFF, dtype=torch.uint8, device=dev) for n in sizes], sizes


def ptr_or_none(t, n):
    return t.data_ptr() if n else None


def run_case(dev, rows, K, integer_round, seed, alloc_extra=2):
    import torch
    lib = _lib.load()
    split = SHAPES[K]
    xb, rb, wb, idx = inputs(rows, K, seed)
    x, r, w, tidx = t_from_bits(xb, dev), t_from_bits(rb, dev), t_from_bits(wb, dev), torch.from_numpy(idx).to(dev)
    flags = _lib.MM_RMS_REFERENCE if integer_round else _lib.MM_RMS_NO_INTEGER_ROUND
    st = torch.cuda.current_stream().cuda_stream
    got, sizes = buffers(rows + alloc_extra, K, split, dev)
    status = lib.mm_add_rmsnorm_quantize(x.data_ptr(), r.data_ptr(), got[0].data_ptr(), w.data_ptr(), EPS, rows, K, tidx.data_ptr(), *split, flags,
                                         *[ptr_or_none(t, n) for t, n in zip(got[1:], sizes[1:])], st)
    assert status == 0, status
    torch.cuda.synchronize()
    s_bits = got[0][:rows * K * 2].cpu().numpy().view(np.uint16).reshape(rows, K)
    want_s = ar.add_bf16(xb, rb)
    assert np.array_equal(s_bits, want_s), f"S_out differs from the rule in {(s_bits != want_s).sum()} elements"
    # the six buffers: byte for byte the existing op on S_out, both from 0xFF-filled buffers of the same size -- which also shows that
    # neither writes a byte the other does not
    plain, _ = buffers(rows + alloc_extra, K, split, dev)
    s_t = t_from_bits(s_bits, dev)
    status = lib.mm_rmsnorm_quantize(s_t.data_ptr(), w.data_ptr(), EPS, rows, K, tidx.data_ptr(), *split, flags,
                                     *[ptr_or_none(t, n) for t, n in zip(plain[1:], sizes[1:])], st)
    assert status == 0, status
    torch.cuda.synchronize()
    for i in range(1, 7):
        a, b = got[i].cpu().numpy(), plain[i].cpu().numpy()
        assert np.array_equal(a, b), f"buffer {i} differs from mm_rmsnorm_quantize(S_out) in {(a != b).sum()} bytes"
    # nothing past `rows`: S_out and the packed segments keep 0xFF behind their last row, the scale tensors outside the rows' offsets
    kn, ks, ko = split
    for t, per_row in ((got[0], K * 2), (got[1], kn // 2), (got[2], ks // 4 * 3), (got[3], ko)):
        if per_row:
            tail = t[rows * per_row:].cpu().numpy()
            assert tail.size >= alloc_extra * per_row and np.all(tail == 0xFF)
    for t, kseg in zip(got[4:], split):
        if kseg:
            sf = t.cpu().numpy().copy()
            sf[o.sf_valid_offsets(rows, kseg)] = 0xFF
            assert np.all(sf == 0xFF), "a scale byte outside the rows' own was written"
    return xb, rb, wb, idx, s_bits, got


@pytest.mark.parametrize("integer_round", (True, False))
@pytest.mark.parametrize("rows", (1, 3))
@pytest.mark.parametrize("K", sorted(SHAPES))
def test_sum_and_buffers(dev, K, rows, integer_round):
    import torch
    xb, rb, wb, idx, s_bits, got = run_case(dev, rows, K, integer_round, seed=K + rows)
    assert s_bits[0, 0] == 0x0002 and s_bits[0, 1] == 0x0080 and s_bits[0, 2] == 0x8080 and s_bits[0, 3] == 0x8001      # subnormal sums survive
    if rows > 1:
        # x = -r: a row of +0 whose bytes are the existing op's zero-block bytes
        assert np.all(s_bits[1] == 0)
        split = SHAPES[K]
        zero = mixedgemm.rmsnorm_quantize_x(torch.zeros((1, K), dtype=torch.bfloat16, device=dev), t_from_bits(wb, dev), EPS,
                                            torch.from_numpy(idx).to(dev), *split, integer_round=integer_round)
        for i, per_row in enumerate((split[0] // 2, split[1] // 4 * 3, split[2])):
            if per_row:
                assert np.array_equal(got[1 + i][per_row:2 * per_row].cpu().numpy(), zero[i][0].cpu().numpy())
        for i, kseg in enumerate(split):
            if kseg:
                assert np.all(got[4 + i].cpu().numpy()[o.sf_valid_offsets(2, kseg)[kseg // 32:]] == 126)
    if rows > 2:
        # +-inf / NaN stay in row 2: inf + 1, -inf + 1, inf - inf, NaN + 0, overflow, 1 - inf
        assert s_bits[2, :6].tolist() == [0x7F80, 0xFF80, 0x7FC0, 0x7FC0, 0x7F80, 0xFF80]
        others = np.delete(s_bits, 2, axis=0)
        assert np.all((others & 0x7F80) != 0x7F80)


@pytest.mark.parametrize("K", (128, 4096))
def test_a_workgroup_walks_several_rows(dev, K):
    rows = many_rows(K)
    run_case(dev, rows, K, True, seed=K)


def test_python_op_returns_the_sum_next_to_the_tuple(dev):
    import torch
    K, rows = 384, 5
    split = SHAPES[K]
    xb, rb, wb, idx = inputs(rows, K, 9)
    x, r, w, tidx = t_from_bits(xb, dev), t_from_bits(rb, dev), t_from_bits(wb, dev), torch.from_numpy(idx).to(dev)
    out = mixedgemm.add_rmsnorm_quantize_x(x, r, w, EPS, tidx, *split)
    assert len(out) == 7
    want = mixedgemm.rmsnorm_quantize_x(out[0], w, EPS, tidx, *split)
    assert np.array_equal(bits_from_t(out[0]), ar.add_bf16(xb, rb))
    for a, b, kseg in zip(out[1:4], want[:3], split):
        assert torch.equal(a, b)
    for a, b, kseg in zip(out[4:], want[3:], split):
        offs = o.sf_valid_offsets(rows, kseg)
        assert np.array_equal(a.cpu().numpy()[offs], b.cpu().numpy()[offs])
    # out_sum: the caller's tensor receives s; one that overlaps an input is refused
    mine = torch.empty_like(x)
    again = mixedgemm.add_rmsnorm_quantize_x(x, r, w, EPS, tidx, *split, out_sum=mine)
    assert again[0] is mine and torch.equal(mine.view(torch.int16), out[0].view(torch.int16))
    with pytest.raises(RuntimeError, match="bad argument"):
        mixedgemm.add_rmsnorm_quantize_x(x, r, w, EPS, tidx, *split, out_sum=x)
    empty = mixedgemm.add_rmsnorm_quantize_x(x[:0], r[:0], w, EPS, tidx, *split)
    assert empty[0].shape == (0, K) and empty[1].shape == (0, split[0] // 2)


def test_overlapping_s_out_is_refused_and_nothing_is_written(dev):
    import torch
    lib = _lib.load()
    K, rows = 384, 3
    split = SHAPES[K]
    xb, rb, wb, idx = inputs(rows, K, 4)
    x, r, w, tidx = t_from_bits(xb, dev), t_from_bits(rb, dev), t_from_bits(wb, dev), torch.from_numpy(idx).to(dev)
    both = torch.cat([x.reshape(-1), r.reshape(-1)])               # x directly in front of r: an S_out in between overlaps both
    xs, rs = both[:rows * K], both[rows * K:]
    got, sizes = buffers(rows, K, split, dev)
    st = torch.cuda.current_stream().cuda_stream
    for s_ptr in (xs.data_ptr(), rs.data_ptr(), xs.data_ptr() + 16, rs.data_ptr() - 16, rs.data_ptr() + rows * K * 2 - 16):
        status = lib.mm_add_rmsnorm_quantize(xs.data_ptr(), rs.data_ptr(), s_ptr, w.data_ptr(), EPS, rows, K, tidx.data_ptr(), *split, 0,
                                             *[ptr_or_none(t, n) for t, n in zip(got[1:], sizes[1:])], st)
        assert status == _lib.MM_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert all(bool((t == 0xFF).all()) for t in got[1:])
    assert np.array_equal(bits_from_t(xs).reshape(rows, K), xb) and np.array_equal(bits_from_t(rs).reshape(rows, K), rb)


def test_operands_at_the_end_of_their_allocations(dev):
    """every operand ending where its own allocation ends (a child process, as tests/test_rope_append_gpu.py does)"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "add_rms_bounds_probe.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "done" in p.stdout, (p.stdout[-1500:], p.stderr[-1500:])
    cases = [l.split() for l in p.stdout.splitlines() if l.startswith("case")]
    assert len(cases) == 3
    for c in cases:
        assert c[-1] == c[-2], c            # the same bytes as with the operands in the middle of torch's pool


# ---- decode entries --------------------------------------------------------------------------------------------------------------------
from test_rmsnorm_decode_gpu import CASES as DECODE_CASES      # (m, n, k, split): M = 1, 2, 3, 4, 5, 7, 8 over both kernel families

NAN_FILL = 0x7FA5        # a NaN no sum produces (the rule's only NaN is 0x7FC0)


def decode_inputs(dev, m, k, seed):
    import torch
    rng = np.random.default_rng(seed)
    xb = o.f32_to_bf16(rng.standard_normal((m, k)).astype(np.float32))
    rb = o.f32_to_bf16((2 * rng.standard_normal((m, k))).astype(np.float32))
    xb[0, :8] = [0x0001, 0x0040, 0x807F, 0x0001, 0x0000, 0x8000, 0x0033, 0x8001]
    rb[0, :8] = [0x0001, 0x0040, 0x8001, 0x8002, 0x0003, 0x0001, 0x0011, 0x8001]
    if m > 1:
        rb[1] = xb[1] ^ 0x8000                                   # a zero row
    nwb = o.f32_to_bf16((1.0 + 0.25 * rng.standard_normal(k)).astype(np.float32))
    idx = rng.permutation(k).astype(np.int16)
    return xb, rb, t_from_bits(xb, dev), t_from_bits(rb, dev), t_from_bits(nwb, dev), torch.from_numpy(idx).to(dev), rng


def sum_buffer(dev, m, k, extra=3):
    """[m + extra, k] of NAN_FILL; the launch gets the first m rows"""
    import torch
    return torch.full((m + extra, k), NAN_FILL, dtype=torch.int16, device=dev).view(torch.bfloat16)


def check_sum(buf, m, xb, rb):
    bits = bits_from_t(buf)
    assert np.array_equal(bits[:m], ar.add_bf16(xb, rb)), "S_out differs from the rule"
    assert np.all(bits[m:] == NAN_FILL), "a row of S_out past M was written"


@pytest.mark.parametrize("wmode", ("w4", "w"))
@pytest.mark.parametrize("m,n,k,split", DECODE_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in DECODE_CASES])
def test_decode_equals_add_rmsnorm_quantize_then_matmul(dev, wmode, m, n, k, split):
    import torch
    xb, rb, x, r, nw, tidx, rng = decode_inputs(dev, m, k, m * 17 + n + k)
    w = t_from_bits(o.f32_to_bf16((0.1 * rng.standard_normal((n, k))).astype(np.float32)), dev)
    bias = t_from_bits(o.f32_to_bf16(rng.standard_normal(n).astype(np.float32)), dev)
    assert mixedgemm.rmsnorm_qlinear_decode_supported(m, n, *split, weight_mode=wmode) >= 1
    b = (mixedgemm.reorder_quantize_w4 if wmode == "w4" else mixedgemm.reorder_quantize_w)(w, tidx, *split)
    for ir in (True, False):
        s, *a = mixedgemm.add_rmsnorm_quantize_x(x, r, nw, EPS, tidx, *split, integer_round=ir)
        for rounding, bv in (("reference", None), ("fused", bias), ("reference", bias)):
            want = mixedgemm.matmul(a[0], b[0], a[1], b[1], a[2], b[2], a[3], b[3], a[4], b[4], a[5], b[5], bias=bv, rounding=rounding)
            buf = sum_buffer(dev, m, k)
            got_s, got = mixedgemm.add_rmsnorm_qlinear_decode(x, r, nw, EPS, tidx, *b, *split, bias=bv, rounding=rounding, integer_round=ir, out_sum=buf[:m])
            torch.cuda.synchronize()
            assert torch.equal(got, want), (m, n, k, split, wmode, ir, rounding)
            check_sum(buf, m, xb, rb)
            assert got_s.data_ptr() == buf.data_ptr()


# one M for each value the query returns, on a narrow layer (the first fused kernel) and a wide one (the streaming kernel)
@pytest.mark.parametrize("m,n,k,split,answer", [(1, 768, 512, (256, 128, 128), 2), (2, 768, 512, (256, 128, 128), 2), (3, 768, 512, (256, 128, 128), 1),
                                                (4, 768, 512, (256, 128, 128), 1), (8, 768, 512, (256, 128, 128), 1), (9, 768, 512, (256, 128, 128), 0),
                                                (1, 8192, 1024, (512, 128, 384), 2), (2, 8192, 1024, (512, 128, 384), 2), (3, 8192, 1024, (512, 128, 384), 1),
                                                (4, 8192, 1024, (512, 128, 384), 1), (8, 8192, 1024, (512, 128, 384), 1)])
def test_decode_for_every_answer_of_the_query(dev, m, n, k, split, answer):
    import torch
    assert mixedgemm.rmsnorm_qlinear_decode_supported(m, n, *split) == answer
    xb, rb, x, r, nw, tidx, rng = decode_inputs(dev, m, k, m + n)
    w = t_from_bits(o.f32_to_bf16((0.1 * rng.standard_normal((n, k))).astype(np.float32)), dev)
    b = mixedgemm.reorder_quantize_w4(w, tidx, *split)
    buf = sum_buffer(dev, m, k)
    if answer == 0:
        with pytest.raises(RuntimeError, match="unsupported"):
            mixedgemm.add_rmsnorm_qlinear_decode(x, r, nw, EPS, tidx, *b, *split, out_sum=buf[:m])
        torch.cuda.synchronize()
        assert np.all(bits_from_t(buf) == NAN_FILL)
        return
    s, *a = mixedgemm.add_rmsnorm_quantize_x(x, r, nw, EPS, tidx, *split)
    want = mixedgemm.matmul(a[0], b[0], a[1], b[1], a[2], b[2], a[3], b[3], a[4], b[4], a[5], b[5])
    _, got = mixedgemm.add_rmsnorm_qlinear_decode(x, r, nw, EPS, tidx, *b, *split, out_sum=buf[:m])
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    check_sum(buf, m, xb, rb)
    with pytest.raises(RuntimeError, match="bad argument"):                 # S_out over X, over R
        mixedgemm.add_rmsnorm_qlinear_decode(x, r, nw, EPS, tidx, *b, *split, out_sum=x)
    with pytest.raises(RuntimeError, match="bad argument"):
        mixedgemm.add_rmsnorm_qlinear_decode(x, r, nw, EPS, tidx, *b, *split, out_sum=r)
    assert np.array_equal(bits_from_t(x), xb) and np.array_equal(bits_from_t(r), rb)


# (m, I, k, split, down split, the query's answer): a narrow MLP (two launches inside the entry) and a wide one (one launch up to M = 4)
GATE_UP = [(1, 256, 256, (128, 0, 128), (128, 0, 128), 1), (3, 256, 512, (256, 128, 128), (0, 128, 128), 1), (8, 512, 512, (256, 128, 128), (256, 128, 128), 1),
           (1, 8192, 1024, (512, 128, 384), (4096, 2048, 2048), 2), (2, 8192, 1024, (512, 128, 384), (4096, 2048, 2048), 2),
           (3, 8192, 1024, (512, 128, 384), (4096, 2048, 2048), 1), (4, 8192, 1024, (512, 128, 384), (4096, 2048, 2048), 1),
           (8, 8192, 1024, (512, 128, 384), (4096, 2048, 2048), 1), (9, 256, 256, (128, 0, 128), (128, 0, 128), 0)]


@pytest.mark.parametrize("m,inter,k,split,dsplit,answer", GATE_UP, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in GATE_UP])
def test_gate_up_decode_equals_add_rmsnorm_quantize_then_gate_up_activate(dev, m, inter, k, split, dsplit, answer):
    import torch
    assert mixedgemm.rmsnorm_gate_up_activate_decode_supported(m, inter, *split) == answer
    xb, rb, x, r, nw, tidx, rng = decode_inputs(dev, m, k, m + inter + k)
    wg = t_from_bits(o.f32_to_bf16((0.1 * rng.standard_normal((inter, k))).astype(np.float32)), dev)
    wu = t_from_bits(o.f32_to_bf16((0.1 * rng.standard_normal((inter, k))).astype(np.float32)), dev)
    gu = mixedgemm.interleave_gate_up(mixedgemm.reorder_quantize_w4(wg, tidx, *split), mixedgemm.reorder_quantize_w4(wu, tidx, *split))
    if answer == 0:
        buf = sum_buffer(dev, m, k)
        with pytest.raises(RuntimeError, match="unsupported"):
            mixedgemm.add_rmsnorm_gate_up_activate_decode(x, r, nw, EPS, tidx, gu, *dsplit, out_sum=buf[:m])
        torch.cuda.synchronize()
        assert np.all(bits_from_t(buf) == NAN_FILL)
        return
    for ir in (True, False):
        for rounding in ("reference", "fused"):
            s, *a = mixedgemm.add_rmsnorm_quantize_x(x, r, nw, EPS, tidx, *split, integer_round=ir)
            want = mixedgemm.gate_up_activate(a, gu, *dsplit, rounding=rounding)
            buf = sum_buffer(dev, m, k)
            _, *got = mixedgemm.add_rmsnorm_gate_up_activate_decode(x, r, nw, EPS, tidx, gu, *dsplit, rounding=rounding, integer_round=ir, out_sum=buf[:m])
            torch.cuda.synchronize()
            for i in range(3):
                assert torch.equal(got[i], want[i]), (i, ir, rounding)
            for i, kseg in enumerate(dsplit):
                offs = o.sf_valid_offsets(m, kseg)
                assert np.array_equal(got[3 + i].cpu().numpy()[offs], want[3 + i].cpu().numpy()[offs]), (i, ir, rounding)
            check_sum(buf, m, xb, rb)
    with pytest.raises(RuntimeError, match="bad argument"):
        mixedgemm.add_rmsnorm_gate_up_activate_decode(x, r, nw, EPS, tidx, gu, *dsplit, out_sum=x)


def test_torchs_device_add_is_the_rule_on_nan_too(dev):
    """the layers' claim 'the same bits as torch adds' on the device: torch's add there, NaN results included"""
    rng = np.random.default_rng(3)
    xb = rng.integers(0, 1 << 16, size=(64, 512), dtype=np.uint32).astype(np.uint16)
    rb = rng.integers(0, 1 << 16, size=(64, 512), dtype=np.uint32).astype(np.uint16)
    xb[0, :3], rb[0, :3] = [0x7F80, 0xFF80, 0x7FC1], [0xFF80, 0x7F80, 0x3F80]
    got = bits_from_t(t_from_bits(xb, dev) + t_from_bits(rb, dev))
    assert np.array_equal(got, ar.add_bf16(xb, rb))


# ---- layers ---------------------------------------------------------------------------------------------------------------------------
H, INTER, SPLIT, DOWN_SPLIT = 512, 1024, (256, 128, 128), (512, 256, 256)


class Layer:
    def __init__(self, dev, g):
        import torch
        idx = torch.randperm(H, generator=g)
        lin = lambda n, k, bias=False: torch.nn.Linear(k, n, bias=bias, dtype=torch.bfloat16).to(dev)
        q = lambda l, i=idx: QLinearLayer(l, p8_num=SPLIT[2], p6_num=SPLIT[1], reorder_index=i)
        self.qkv = FusedQLinear([q(lin(512, H, True)), q(lin(128, H, True)), q(lin(128, H, True))])
        self.o = q(lin(H, H), torch.randperm(H, generator=g))
        idx2 = torch.randperm(H, generator=g)
        self.mlp = FusedMLP(q(lin(INTER, H), idx2), q(lin(INTER, H), idx2), (0.05 * torch.randn((H, INTER), generator=g)).to(torch.bfloat16), DOWN_SPLIT)
        self.w_in = (1 + 0.1 * torch.randn((H,), generator=g)).to(torch.bfloat16).to(dev)
        self.w_post = (1 + 0.1 * torch.randn((H,), generator=g)).to(torch.bfloat16).to(dev)


def attention_stand_in(q, k, v):
    """not attention: something elementwise that mixes q, k and v into [.., H]"""
    return q * 0.5 + k.repeat(1, 1, 4) * 0.25 + v.repeat(1, 1, 4)


def chain(layers, x, fused):
    """two decoder layers; `fused`: the residual adds ride inside forward_norm / FusedMLP.forward, else torch adds in front of them"""
    s = mlp_out = None
    for n, l in enumerate(layers):
        if n == 0:
            s = x
            qkv = l.qkv.forward_norm(x, l.w_in, EPS)                       # the first norm has no add in front of it
        elif fused:
            qkv, s = l.qkv.forward_norm(mlp_out, l.w_in, EPS, residual=s)  # the previous layer's second add, in this layer's input norm
        else:
            s = mlp_out + s
            qkv = l.qkv.forward_norm(s, l.w_in, EPS)
        a = l.o(attention_stand_in(*qkv))
        if fused:
            mlp_out, s = l.mlp(a, l.w_post, EPS, residual=s)
        else:
            s = a + s
            mlp_out = l.mlp(s, l.w_post, EPS)
    return mlp_out, s


@pytest.fixture(scope="module")
def layers(dev):
    import torch
    g = torch.Generator().manual_seed(21)
    return [Layer(dev, g), Layer(dev, g)]


@pytest.mark.parametrize("m", (1, 16))
def test_threading_the_residual_equals_torch_adds(dev, layers, m):
    """m = 1: the one-launch decode forms with the add inside (where the query answers 2); m = 16: the two-launch form, with the add inside
    the quantizer"""
    import torch
    assert mixedgemm.rmsnorm_qlinear_decode_supported(1, 768, *SPLIT) == 2 and mixedgemm.rmsnorm_qlinear_decode_supported(16, 768, *SPLIT) != 2
    x = torch.randn((1, m, H), generator=torch.Generator().manual_seed(m)).to(torch.bfloat16).to(dev)
    y1, s1 = chain(layers, x, True)
    y0, s0 = chain(layers, x, False)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y0.float()).all()) and float(y0.float().abs().max()) > 0
    assert y1.shape == y0.shape == (1, m, H) and s1.shape == s0.shape == (1, m, H)
    assert torch.equal(y1.view(torch.int16), y0.view(torch.int16)) and torch.equal(s1.view(torch.int16), s0.view(torch.int16))


def test_without_a_residual_nothing_changes(dev, layers):
    import torch
    l = layers[0]
    for m in (1, 16):
        x = torch.randn((1, m, H), generator=torch.Generator().manual_seed(40 + m)).to(torch.bfloat16).to(dev)
        r = torch.zeros_like(x)
        qkv = l.qkv.forward_norm(x, l.w_in, EPS)
        assert isinstance(qkv, tuple) and len(qkv) == 3 and all(isinstance(t, torch.Tensor) for t in qkv)
        with_r, s = l.qkv.forward_norm(x, l.w_in, EPS, residual=r)            # x + 0 = x: the same bits through the other path
        assert all(torch.equal(a, b) for a, b in zip(qkv, with_r)) and torch.equal(s, x)
        y = l.o.forward_norm(x, l.w_in, EPS)
        assert isinstance(y, torch.Tensor) and y.shape == (1, m, H)
        y_r, s = l.o.forward_norm(x, l.w_in, EPS, residual=r)
        assert torch.equal(y, y_r) and torch.equal(s, x)
        z = l.mlp(x, l.w_post, EPS)
        assert isinstance(z, torch.Tensor) and z.shape == (1, m, H)
        z_r, s = l.mlp(x, l.w_post, EPS, residual=r)
        assert torch.equal(z, z_r) and torch.equal(s, x)
        x2 = x.reshape(m, H)                                                  # the 2-D caller form
        y2, s2 = l.o.forward_norm(x2, l.w_in, EPS, residual=r.reshape(m, H))
        assert y2.shape == (m, H) and s2.shape == (m, H) and torch.equal(y2, y.reshape(m, H))
    with pytest.raises(ValueError):
        l.mlp(x, residual=r)


def test_graph_capture_of_the_chain_with_residuals(dev, layers):
    import torch
    static = torch.randn((1, 1, H), generator=torch.Generator().manual_seed(60)).to(torch.bfloat16).to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            chain(layers, static, True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = chain(layers, static, True)
    for seed in (61, 62):
        x = torch.randn((1, 1, H), generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16).to(dev)
        static.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        want = chain(layers, x, True)
        torch.cuda.synchronize()
        assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])


class CountingLib:
    """stands in for the ctypes handle: counts the calls of every mm_* entry (as tests/test_moe_device_sized_gpu.py)"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("mm_"):
            return fn

        def counted(*a):
            self.calls.append(name)
            return fn(*a)
        return counted


@pytest.mark.parametrize("m", (1, 16))
def test_no_more_library_calls_with_residuals(dev, layers, monkeypatch, m):
    """m = 1: the one-launch decode forms; m = 16: quantizer + GEMM.  With residuals the launch that holds the norm is its add_ form, and
    the count is the same -- the adds cost no call of their own"""
    import torch
    x = torch.randn((1, m, H), generator=torch.Generator().manual_seed(70)).to(torch.bfloat16).to(dev)
    seen = {}
    for fused in (False, True):
        counting = CountingLib(_lib.load())
        monkeypatch.setattr(_lib, "_lib", counting)
        for l in layers:                                                     # the per-layer plans keep the handle they were built with
            for mod in (l.qkv, l.o):
                mod.__dict__.pop("_decode_plan", None)
        try:
            chain(layers, x, fused)
            torch.cuda.synchronize()
        finally:
            monkeypatch.undo()
            for l in layers:
                for mod in (l.qkv, l.o):
                    mod.__dict__.pop("_decode_plan", None)
        seen[fused] = [c for c in counting.calls if not c.endswith("_supported") and not c.endswith("_supported_w") and not c.endswith("_bytes")
                       and c != "mm_sf_bytes_x"]
    assert len(seen[True]) == len(seen[False]), seen
    adds = lambda calls: [c for c in calls if c.startswith("mm_add_")]
    assert not adds(seen[False])
    if m == 1:
        assert adds(seen[True]) == ["mm_add_rmsnorm_qlinear_decode"] * 3, seen
    else:
        assert adds(seen[True]) == ["mm_add_rmsnorm_quantize"] * 3, seen
