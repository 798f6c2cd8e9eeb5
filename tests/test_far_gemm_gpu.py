"""GPU tests of the GEMM epilogue, the activation quantizers and the MoE row movers at sizes where a row's offset passes 2^31 / 2^32
bytes and 2^31 / 2^32 elements (tests/far_cases.py holds the shapes, tests/test_far_cpu.py the thresholds each crosses):

matmul      M = 66048, N = 65536, K = (128, 128, 128), fp4 weights, bias: a bf16 output of 8.06 GiB.  On the device the whole output is
            bit-equal to the same operands run in chunks of 4096 rows (every chunk re-quantized from its rows of X: the quantizers
            work row by row); on the host check_gemm holds the first, the last and the rows on both sides of every threshold to the
            oracle, which quantizes those rows itself.  The same with out_dtype = fp32 at M = 16640 (4.06 GiB), chunks only
quantizers  reorder_quantize_x and rmsnorm_quantize_x at K = 32768, rows = 65664 (an input of 4.01 GiB), splits (0, 0, 32768) -- the
            fp8 output passes 2^31 bytes -- and (16384, 8192, 8192): the oracle's bytes and scale bytes on the probe rows, and the
            whole output against chunks of 8192 rows
activate    activate_quantize_x on gate and up of that shape (the smallest multiple of 128 rows whose input passes 2^31 elements), row r
            holding row r % 509 of tests/act_exact_cases.py's lossless family, on which the oracle's bytes are exact: held the same way
moe         moe_gather from x [131080, 32768] and moe_combine over y_sorted of that shape (top_k 8, T = 16385) in one 8 GiB buffer from
            torch.empty of which only the rows named are filled: the probe rows and the rows their offsets wrap to.  Both kernels
            count rows in 16-byte vectors, so a 32-bit `t * V` would wrap only at 32 GiB: the 64-bit pointer sums are what runs here

Each group is a class whose fixture is released before the next group's is made: the file holds one group's buffers at a time."""
import numpy as np
import pytest
import torch

from micromix_amd import _lib, mixedgemm
from micromix_amd import moe_ops
from oracle import mx_oracle as o
import act_exact_cases as ac
import far_cases as fc
import gemm_check
import moe_oracle as mo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def memory(dev):
    need, free = fc.gemm_need_bytes(), torch.cuda.mem_get_info(dev)[0]
    if free < need:
        pytest.skip(f"the far GEMM tests need {need / fc.GIB:.1f} GiB of device memory (tests/far_cases.py), {free / fc.GIB:.1f} GiB are free")
    yield
    torch.cuda.empty_cache()


def bits_of(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def randn_bf16(shape, seed, dev, scale=1.0):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=dev, dtype=torch.float32) * scale).to(torch.bfloat16)


# ---- matmul ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="class")
def gemm_operands(dev):
    kn, ks, ko = fc.GEMM_SPLIT
    k = kn + ks + ko
    x = randn_bf16((fc.GEMM_M, k), 1, dev)
    x[:, ::50] *= 20.0
    w = randn_bf16((fc.GEMM_N, k), 2, dev, 0.02)
    idx = torch.randperm(k, generator=torch.Generator().manual_seed(3)).to(torch.int16).to(dev)
    bias = randn_bf16((fc.GEMM_N,), 4, dev)
    qw = mixedgemm.reorder_quantize_w4(w, idx, kn, ks, ko)
    box = dict(x=x, w=w, idx=idx, bias=bias, qw=qw)
    yield box
    box.clear()
    torch.cuda.empty_cache()


def run_matmul(c, rows, **kw):
    qx = mixedgemm.reorder_quantize_x(c["x"][rows], c["idx"], *fc.GEMM_SPLIT)
    qw = c["qw"]
    return mixedgemm.matmul(qx[0], qw[0], qx[1], qw[1], qx[2], qw[2], qx[3], qw[3], qx[4], qw[4], qx[5], qw[5], **kw)


def assert_chunks_equal(c, out, M, **kw):
    view = torch.int16 if out.dtype is torch.bfloat16 else torch.int32
    for r0 in range(0, M, fc.GEMM_CHUNK):
        rows = slice(r0, min(r0 + fc.GEMM_CHUNK, M))
        part = run_matmul(c, rows, **kw)
        bad = (part.view(view) != out[rows].view(view)).any(dim=1)
        assert not bool(bad.any()), f"rows {r0 + int(bad.nonzero()[0])} .. of the whole output differ from the chunk's ({int(bad.sum())} rows)"


class TestMatmul:
    def test_matmul_bf16_output_past_every_threshold(self, dev, gemm_operands):
        c, M, N = gemm_operands, fc.GEMM_M, fc.GEMM_N
        kn, ks, ko = fc.GEMM_SPLIT
        lib = _lib.load()
        flags = _lib.MM_ROUND_PER_SEGMENT | _lib.MM_WS_TICKETS_ZEROED
        ws = lib.mm_matmul_workspace_bytes(M, N, kn, ks, ko, _lib.MM_W_FP4, flags)
        print(f"dispatch of M {M} N {N} K {fc.GEMM_SPLIT}: {lib.mm_matmul_describe(M, N, kn, ks, ko, _lib.MM_W_FP4, flags, ws).decode()}")
        out = run_matmul(c, slice(0, M), bias=c["bias"])
        assert out.numel() * 2 == fc.GEMM_OUT.nbytes() > fc.B32 and out.numel() > fc.E32
        assert_chunks_equal(c, out, M, bias=c["bias"])
        rows = fc.GEMM_OUT.probe_rows()
        sel = torch.tensor(rows, device=dev)
        idx = c["idx"].cpu().numpy()
        qx = o.reorder_quantize(bits_of(c["x"][sel]), idx, kn, ks, ko, "x")
        qw = o.reorder_quantize(bits_of(c["w"]), idx, kn, ks, ko, "w4")
        gemm_check.check_gemm(bits_of(out[sel]), qx, qw, rounding="reference", bias_bits=bits_of(c["bias"]), label=f"rows {rows}")


    def test_matmul_fp32_output_past_b32(self, dev, gemm_operands):
        c, M = gemm_operands, fc.GEMM_F32_M
        kw = dict(rounding="fused", out_dtype=torch.float32)
        out = run_matmul(c, slice(0, M), **kw)
        assert out.dtype is torch.float32 and out.numel() * 4 == fc.GEMM_OUT_F32.nbytes() > fc.B32
        assert_chunks_equal(c, out, M, **kw)
        # the fp32 sums, rounded once, are the bf16 output of the same call
        rows = torch.tensor(fc.GEMM_OUT_F32.probe_rows(), device=dev)
        qx = mixedgemm.reorder_quantize_x(c["x"][rows], c["idx"], *fc.GEMM_SPLIT)
        qw = c["qw"]
        small = mixedgemm.matmul(qx[0], qw[0], qx[1], qw[1], qx[2], qw[2], qx[3], qw[3], qx[4], qw[4], qx[5], qw[5], rounding="fused")
        assert torch.equal(out[rows].to(torch.bfloat16).view(torch.int16), small.view(torch.int16))


# ---- quantizers ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="class")
def quant_input(dev):
    x = torch.empty((fc.QUANT_ROWS, fc.QUANT_K), dtype=torch.bfloat16, device=dev)
    for r0 in range(0, fc.QUANT_ROWS, fc.QUANT_CHUNK):                       # every row its own values
        x[r0: r0 + fc.QUANT_CHUNK] = randn_bf16(tuple(x[r0: r0 + fc.QUANT_CHUNK].shape), 100 + r0, dev, 2.0)
    box = dict(x=x, idx=torch.randperm(fc.QUANT_K, generator=torch.Generator().manual_seed(5)).to(torch.int16).to(dev),
               w=(1 + 0.1 * randn_bf16((fc.QUANT_K,), 6, dev).float()).to(torch.bfloat16))
    assert x.numel() > fc.E31 and x.numel() * 2 > fc.B32
    yield box
    box.clear()
    torch.cuda.empty_cache()


def hold_quantizer(call, inputs, want, rows, split, label):
    """the six outputs of call(*inputs) over every row: the oracle's packed bytes and scale bytes (`want`, computed on `rows` alone) at
    those rows' places in the whole tensors, and the whole output against the same rows run in chunks -- a chunk of whole 128-row tiles is
    a contiguous slice of every tensor.  Returns the whole output."""
    whole = call(*inputs)
    dev, total = inputs[0].device, inputs[0].shape[0]
    sel = torch.tensor(rows, device=dev)
    for seg, kseg in enumerate(split):
        if not kseg:
            continue
        assert np.array_equal(whole[seg][sel].cpu().numpy(), want[seg]), f"{label}: packed bytes of segment {seg} on rows {rows}"
        j = np.arange(kseg // 32)[None, :]
        local = want[3 + seg][o.sf_offset(np.arange(len(rows))[:, None], j, kseg)]
        at = torch.from_numpy(o.sf_offset(np.array(rows)[:, None], j, kseg)).to(dev)
        assert np.array_equal(whole[3 + seg][at].cpu().numpy(), local), f"{label}: scale bytes of segment {seg} on rows {rows}"
    for r0 in range(0, total, fc.QUANT_CHUNK):
        r1 = min(r0 + fc.QUANT_CHUNK, total)
        part = call(*(t[r0:r1] for t in inputs))
        for seg, kseg in enumerate(split):
            if kseg:
                assert torch.equal(part[seg], whole[seg][r0:r1]), f"{label}: packed rows {r0} .. {r1} of segment {seg}"
                n = (r1 - r0) // 128 * (kseg // 128) * 512
                s0 = r0 // 128 * (kseg // 128) * 512
                assert torch.equal(part[3 + seg][:n], whole[3 + seg][s0: s0 + n]), f"{label}: scales of rows {r0} .. {r1} of segment {seg}"
    return whole


class TestQuantizers:
    @pytest.mark.parametrize("split", fc.QUANT_SPLITS, ids=["all_fp8", "mixed"])
    @pytest.mark.parametrize("op", ["reorder", "rmsnorm"])
    def test_quantizers_on_an_input_past_e31(self, dev, quant_input, op, split):
        c, eps = quant_input, 1e-5
        call = (lambda x: mixedgemm.reorder_quantize_x(x, c["idx"], *split)) if op == "reorder" else \
            (lambda x: mixedgemm.rmsnorm_quantize_x(x, c["w"], eps, c["idx"], *split))
        rows = fc.QUANT_IN.probe_rows()
        xb, idx = bits_of(c["x"][torch.tensor(rows, device=dev)]), c["idx"].cpu().numpy()
        want = o.reorder_quantize(xb, idx, *split, "x") if op == "reorder" else o.rmsnorm_quantize(xb, bits_of(c["w"]), eps, idx, *split)
        whole = hold_quantizer(call, (c["x"],), want, rows, split, f"{op} {split}")
        if split[0] == 0:
            assert whole[2].numel() == fc.QUANT_OUT_FP8.nbytes() > fc.B31


# ---- activate_quantize_x ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="class")
def act_buffers(dev):
    """gate and up, [65664, 32768] bf16 each, from torch.empty; a test fills them"""
    box = dict(gate=torch.empty((fc.ACT_ROWS, fc.ACT_K), dtype=torch.bfloat16, device=dev),
               up=torch.empty((fc.ACT_ROWS, fc.ACT_K), dtype=torch.bfloat16, device=dev))
    yield box
    box.clear()
    torch.cuda.empty_cache()


class TestActivate:
    @pytest.mark.parametrize("split", fc.QUANT_SPLITS, ids=["all_fp8", "mixed"])
    def test_activate_quantize_x_on_inputs_past_e31(self, dev, act_buffers, split):
        gate, up = ac.family(fc.ACT_PERIOD, split)                          # the lossless family: the oracle's bytes are exact on it
        which = torch.arange(fc.ACT_ROWS, device=dev) % fc.ACT_PERIOD
        for name, bits in (("gate", gate), ("up", up)):
            base = torch.from_numpy(bits.view(np.int16)).to(dev).view(torch.bfloat16)
            for r0 in range(0, fc.ACT_ROWS, fc.QUANT_CHUNK):
                act_buffers[name][r0: r0 + fc.QUANT_CHUNK] = base[which[r0: r0 + fc.QUANT_CHUNK]]
        assert act_buffers["gate"].numel() > fc.E31 and act_buffers["gate"].numel() * 2 > fc.B32
        rows = fc.ACT_IN.probe_rows()
        at = np.array(rows) % fc.ACT_PERIOD
        assert len({gate[i].tobytes() + up[i].tobytes() for i in at}) == len(rows)                  # every probe row its own content
        want = o.activate_quantize(gate[at], up[at], *split)
        hold_quantizer(lambda a, b: mixedgemm.activate_quantize_x(a, b, *split), (act_buffers["gate"], act_buffers["up"]), want, rows, split,
                       f"activate_quantize_x {split}")


# ---- MoE rows --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="class")
def moe_buffer(dev):
    """[131080, 32768] bf16 from torch.empty; the rows of far_cases.moe_rows() filled, each with its own values"""
    rows = fc.moe_rows()
    buf = torch.empty((fc.MOE_ROWS, fc.MOE_H), dtype=torch.bfloat16, device=dev)
    content = randn_bf16((len(rows), fc.MOE_H), 7, dev)
    for i, r in enumerate(rows):
        buf[r] = content[i]
    assert len({bytes(b) for b in bits_of(content[:, :64])}) == len(rows)
    box = dict(buf=buf, rows=rows, content=content)
    yield box
    box.clear()
    torch.cuda.empty_cache()


class TestMoE:
    def test_moe_gather_from_rows_past_e31_and_e32(self, dev, moe_buffer):
        c = moe_buffer
        rows = c["rows"]
        order = np.random.default_rng(8).permutation(len(rows))
        token = np.concatenate([[rows[i] for i in order], [-1, fc.MOE_ROWS]]).astype(np.int32)          # the last two name no row
        out = torch.full((len(token), fc.MOE_H), 7.0, dtype=torch.bfloat16, device=dev)
        moe_ops.moe_gather(c["buf"], torch.from_numpy(token).to(dev), out=out)
        assert torch.equal(out[: len(rows)].view(torch.int16), c["content"][torch.from_numpy(order).to(dev)].view(torch.int16))
        assert bool((out[len(rows):] == 7.0).all()), "a row whose token lies outside [0, T) was written"


    def test_moe_combine_over_slots_past_e31_and_e32(self, dev, moe_buffer):
        c = moe_buffer
        rows, T, k = c["rows"], fc.MOE_T, fc.MOE_TOP_K
        rng = np.random.default_rng(9)
        tokens = [0, 1, T // 2, T - 2, T - 1]
        slot_of = np.full((T, k), -1, dtype=np.int32)
        compact = np.full((T, k), -1, dtype=np.int32)                                  # the same slots as rows of `content`
        for t in tokens:                                                               # five to eight of the named rows per token
            pick = rng.choice(len(rows), size=int(rng.integers(5, k + 1)), replace=False)
            at = rng.permutation(k)[: len(pick)]
            slot_of[t, at] = [rows[i] for i in pick]
            compact[t, at] = pick
        used = {int(s) for s in slot_of[slot_of >= 0]}
        assert {fc.MOE_X.first_row_past(t) for t in ("B31", "E31", "E32")} | {fc.MOE_ROWS - 1} <= used
        ids = np.stack([rng.permutation(64)[:k] for _ in range(T)]).astype(np.int32)
        w = o.f32_to_bf16(rng.random((T, k)).astype(np.float32))
        out = moe_ops.moe_combine(c["buf"], torch.from_numpy(ids).to(dev), torch.from_numpy(w.view(np.int16)).to(dev).view(torch.bfloat16),
                                  torch.from_numpy(slot_of).to(dev))
        want = mo.combine(bits_of(c["content"]), ids[tokens], w[tokens], compact[tokens])
        sel = torch.tensor(tokens, device=dev)
        assert np.array_equal(bits_of(out[sel]), want), "moe_combine on the tokens whose slots lie past the thresholds"
        assert int(torch.count_nonzero(out.view(torch.int16))) == int(np.count_nonzero(want)), "a token without slots is not +0.0 everywhere"


