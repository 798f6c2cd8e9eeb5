"""The decode launches that carry the RMSNorm -- rmsnorm_qlinear_decode and add_rmsnorm_qlinear_decode, in the fused kernel (N = 128)
and in the streaming kernel (N = 8192 at M <= 4; both its early-request path and, at M K / 32 > 512, its hook path), and
rmsnorm_gate_up_activate_decode with its add_ form on a narrow and a wide layer -- on token rows that notice a wrongly ordered sum of squares (tests/golden/rms_sentinels.json, tests/rms_order_cases.py).

Want side: `matmul` of the ORACLE's codes of the token rows with the library-packed weights, bit for bit.  (The existing tests compare
with the library's own quantizer, which shares the order under test.)  Output feature f of the weights is one-hot at the recorded
flip column of sentinel f, so the one code that a wrong order flips reaches an output element by itself
(tests/test_rms_sentinels_cpu.py shows that this element then differs); the other features are random."""
import numpy as np
import pytest

import rms_order_cases as c
from conftest import t_from_bits
from micromix_amd import mixedgemm
from oracle import mx_oracle as o
from test_matmul_gpu import to_dev
from test_rms_order_gpu import block

pytestmark = pytest.mark.gpu
KS = (128, 4096, 4224, 8192)
R0 = 37


def sentinels_of(k):
    """[(integer_round, row of block(k, integer_round, R0), flip column)] over both roundings: entry f owns output feature f"""
    fix = c.load_fixture()
    out = []
    for ir in (True, False):
        for i, n in enumerate(c.sentinel_rows(fix, k, ir)):
            col = next(s["column"] for s in fix["sentinels"] if (s["K"], s["integer_round"], s["row"]) == (k, ir, n))
            out.append((ir, i, col))
    return out


def weights(dev, k, n, wmode):
    import torch
    g = torch.Generator(device=dev).manual_seed(k + n)
    w = (0.1 * torch.randn((n, k), generator=g, device=dev)).to(torch.bfloat16)
    idx = c.reorder_index(k).astype(np.int64)
    owners = sentinels_of(k)
    assert len(owners) <= 128 <= n
    for f, (_, _, col) in enumerate(owners):
        w[f] = 0
        w[f, int(idx[col])] = 1.0                       # reordered position `col`
    tidx = torch.from_numpy(c.reorder_index(k)).to(dev)
    return (mixedgemm.reorder_quantize_w4 if wmode == "w4" else mixedgemm.reorder_quantize_w)(w, tidx, *c.SPLITS[k]), tidx


def oracle_codes(k, integer_round, sel):
    """the oracle's six outputs for rows `sel` of the block, as the arrays a launch of len(sel) rows produces"""
    _, _, packed, scales = block(k, integer_round, R0)
    m = len(sel)
    sfs = []
    for sc, kseg in zip(scales, c.SPLITS[k]):
        sf = np.zeros((o.sf_size_x(m, kseg),), np.uint8)
        if kseg:
            sf[o.sf_valid_offsets(m, kseg)] = sc[sel].reshape(-1)
        sfs.append(sf)
    return [np.ascontiguousarray(p[sel]) for p in packed] + sfs


def token_rows(count, m):
    """the sentinels that are the token rows of the launches at M = m: chunks of m that walk through all of them (the last chunk wraps
    around), so every sentinel meets every M and, whenever M > 1, the last row holds a different one than row 0"""
    return [[(s + i) % count for i in range(m)] for s in range(0, count, m)]


@pytest.mark.parametrize("wmode", ("w4", "w"))
@pytest.mark.parametrize("n,ms", ((128, (1, 3, 8)), (8192, (1, 3))), ids=("fused", "streaming"))
@pytest.mark.parametrize("k", KS)
def test_decode_launches_match_matmul_of_the_oracles_codes(dev, k, n, ms, wmode):
    import torch
    split = c.SPLITS[k]
    b, tidx = weights(dev, k, n, wmode)
    nw = t_from_bits(c.norm_weight(k), dev)
    fix = c.load_fixture()
    for ir in (True, False):
        xb = block(k, ir, R0)[0]
        count = len(c.sentinel_rows(fix, k, ir))
        hb = o.f32_to_bf16(o.bf16_to_f32(xb) * np.float32(0.5))          # x = res = s / 2: the sum is s exactly
        for m in ms:
            assert mixedgemm.rmsnorm_qlinear_decode_supported(m, n, *split, weight_mode=wmode) >= 1
            for sel in token_rows(count, m):
                a = to_dev(dev, oracle_codes(k, ir, sel))
                want = mixedgemm.matmul(a[0], b[0], a[1], b[1], a[2], b[2], a[3], b[3], a[4], b[4], a[5], b[5])
                x, h = t_from_bits(xb[sel], dev), t_from_bits(hb[sel], dev)
                got = mixedgemm.rmsnorm_qlinear_decode(x, nw, c.EPS, tidx, *b, *split, integer_round=ir)
                s, got_add = mixedgemm.add_rmsnorm_qlinear_decode(h, h.clone(), nw, c.EPS, tidx, *b, *split, integer_round=ir)
                torch.cuda.synchronize()
                label = (k, n, wmode, ir, m, sel)
                assert torch.equal(got, want), ("plain", label, torch.nonzero((got != want).any(dim=0)).flatten()[:8].tolist())
                assert torch.equal(s.view(torch.int16), x.view(torch.int16)), label
                assert torch.equal(got_add, want), ("add", label, torch.nonzero((got_add != want).any(dim=0)).flatten()[:8].tolist())


def gate_up_weights(dev, k, inter):
    """gate | up of `inter` features each, interleaved as the launch takes them; gate and up feature f are one-hot at the flip column of
    sentinel f (h_f = silu(v) v of the one element v), the rest random"""
    import torch
    g = torch.Generator(device=dev).manual_seed(k + inter)
    idx = c.reorder_index(k).astype(np.int64)
    tidx = torch.from_numpy(c.reorder_index(k)).to(dev)
    halves = []
    for _ in range(2):
        w = (0.8 * torch.randn((inter, k), generator=g, device=dev)).to(torch.bfloat16)
        for f, (_, _, col) in enumerate(sentinels_of(k)):
            w[f] = 0
            w[f, int(idx[col])] = 1.0
        halves.append(mixedgemm.reorder_quantize_w4(w, tidx, *c.SPLITS[k]))
    return mixedgemm.interleave_gate_up(*halves), tidx


# (I, the down projection's split): the narrow and the wide layer of tests/test_gate_up_gpu.py / tests/test_add_rmsnorm_gpu.py
GATE_UP = ((256, (128, 0, 128)), (8192, (4096, 2048, 2048)))


@pytest.mark.parametrize("inter,dsplit", GATE_UP, ids=("narrow", "wide"))
@pytest.mark.parametrize("k", KS)
def test_gate_up_decode_launches_match_gate_up_activate_of_the_oracles_codes(dev, k, inter, dsplit):
    import torch
    split = c.SPLITS[k]
    gu, tidx = gate_up_weights(dev, k, inter)
    nw = t_from_bits(c.norm_weight(k), dev)
    fix = c.load_fixture()
    for ir in (True, False):
        xb = block(k, ir, R0)[0]
        count = len(c.sentinel_rows(fix, k, ir))
        hb = o.f32_to_bf16(o.bf16_to_f32(xb) * np.float32(0.5))
        for m in (1, 3, 8):
            assert mixedgemm.rmsnorm_gate_up_activate_decode_supported(m, inter, *split) >= 1
            for sel in token_rows(count, m):
                a = to_dev(dev, oracle_codes(k, ir, sel))
                x, h = t_from_bits(xb[sel], dev), t_from_bits(hb[sel], dev)
                for rounding in ("reference", "fused"):
                    want = mixedgemm.gate_up_activate(a, gu, *dsplit, rounding=rounding)
                    got = mixedgemm.rmsnorm_gate_up_activate_decode(x, nw, c.EPS, tidx, gu, *dsplit, rounding=rounding, integer_round=ir)
                    s, *got_add = mixedgemm.add_rmsnorm_gate_up_activate_decode(h, h.clone(), nw, c.EPS, tidx, gu, *dsplit, rounding=rounding,
                                                                                integer_round=ir)
                    torch.cuda.synchronize()
                    label = (k, inter, ir, m, sel, rounding)
                    assert torch.equal(s.view(torch.int16), x.view(torch.int16)), label
                    for form, outs in (("plain", got), ("add", got_add)):
                        for i, kseg in enumerate(dsplit):
                            assert torch.equal(outs[i], want[i]), (form, label, i)
                            offs = torch.from_numpy(o.sf_valid_offsets(m, kseg)).to(dev)
                            assert torch.equal(outs[3 + i][offs], want[3 + i][offs]), (form, label, "scales", i)
