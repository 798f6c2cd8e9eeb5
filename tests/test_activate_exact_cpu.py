"""What tests/test_activate_exact_gpu.py rests on, proved from the oracle alone (no GPU): the lossless gate family really is lossless
and really sits on every edge it claims (tests/act_exact_cases.py), and the admissible-set check of the Gaussian cases is not vacuous."""
import numpy as np
import pytest

import act_exact_cases as ac
from oracle import mx_oracle as o


def exact_product(gate, up):
    return o.bf16_to_f32(gate).astype(np.float64) * o.bf16_to_f32(up).astype(np.float64)


def test_oracle_silu_mul_is_the_exact_product_from_gate_20_on():
    """every bf16 gate in [20, 2^16) against ups with full significands, both signs and zero: o.silu_mul == gate * up bit for bit"""
    allb = np.arange(65536, dtype=np.uint16)
    x = o.bf16_to_f32(allb)
    gate = allb[(x >= ac.GATE_MIN) & (x < 65536.0)]
    for up in (0x3F80, 0xBF80, 0x3FFF, 0xC0D5, 0x2B9B, 0x0000, 0x8000):
        ub = np.full_like(gate, up)
        v = o.silu_mul(gate, ub)
        assert np.array_equal(v.view(np.uint32), exact_product(gate, ub).astype(np.float32).view(np.uint32)), hex(up)
        assert np.array_equal(v.astype(np.float64), exact_product(gate, ub))


@pytest.mark.parametrize("rows,k,split", ac.CASES + [(64, ac.LARGE[1], ac.LARGE[2])])
def test_family_is_lossless(rows, k, split):
    gate, up = ac.family(rows, split)
    assert gate.shape == (rows, k) and float(o.bf16_to_f32(gate).min()) >= 32.0
    p = exact_product(gate, up)
    v = p.astype(np.float32)
    assert np.array_equal(v.astype(np.float64), p)                                   # 16 significand bits: exact in fp32
    want, direct = o.activate_quantize(gate, up, *split), o.direct_quantize(v, *split)
    assert all(np.array_equal(a, b) for a, b in zip(want, direct))
    # a pure function of (row, column): later rows do not depend on the row count
    g2, u2 = ac.family(3, split, row0=rows - 3)
    assert np.array_equal(g2, gate[-3:]) and np.array_equal(u2, up[-3:])


def segment_views(gate, up, split):
    col = 0
    for kseg, fmt in zip(split, ac.FMTS):
        if kseg:
            v = exact_product(gate[:, col:col + kseg], up[:, col:col + kseg]).reshape(len(gate), kseg // 32, 32)
            yield fmt, v
        col += kseg


@pytest.mark.parametrize("fmt", ac.FMTS)
def test_every_edge_occurs(fmt):
    """in the (130, 1024, (512, 128, 384)) case alone, for each format: every midpoint as an exact tie and with a neighbour on either
    side closer than half a bf16 ulp, in both signs; amax == FMAX 2^k, just above and just below it; amax on either side of 1e-6f with
    byte 127 and zero codes below; a zero block with both zeros; a value rounding up onto the largest code; exponents -20 .. 20"""
    rows, k, split = ac.CASES[2]
    gate, up = ac.family(rows, split)
    v = dict(segment_views(gate, up, split))[fmt]
    f = o.FORMATS[fmt]
    fmax = f["fmax"]
    amax = np.abs(v).max(-1)
    e = o.scale_exponent_f32(amax.astype(np.float32), fmt)
    q = v * np.exp2(-e.astype(np.float64))[..., None]
    live = (amax > float(ac.F32_1EM6))[..., None] & np.ones_like(q, bool)
    half = 2.0 ** -9                                                                    # half a bf16 ulp, relative
    for m in ac.midpoints(fmt):
        for s in (1.0, -1.0):
            x = s * q[live]
            assert (x == m).any(), (fmt, m, s, "tie")
            assert ((x > m * (1 - half)) & (x < m)).any(), (fmt, m, s, "below")
            assert ((x > m) & (x < m * (1 + half))).any(), (fmt, m, s, "above")
    r = amax / (fmax * np.exp2(e.astype(np.float64)))                                   # amax / (FMAX * scale), <= 1
    big = amax > float(ac.F32_1EM6)
    assert (r[big] == 1.0).any() and ((r[big] > 1 - half) & (r[big] < 1)).any()
    assert ((r[big] > 0.5) & (r[big] < 0.5 * (1 + half))).any()                         # one product above FMAX * 2^(e - 1)
    assert r[big].max() <= 1.0
    thr = float(ac.F32_1EM6)
    below = (amax > 0.99 * thr) & (amax <= thr)
    assert below.any() and ((amax > thr) & (amax < 1.01 * thr)).any()
    assert (amax == 0).any() and np.signbit(v[amax == 0]).any() and not np.signbit(v[amax == 0]).all()
    assert {-20, 20} <= set(e[big & (r == 1.0)].tolist())                              # block scales 2^-20 .. 2^20 times the format's own
    # what the oracle makes of them
    col = sum(split[:ac.FMTS.index(fmt)])
    want = o.activate_quantize(gate, up, *split)
    i = ac.FMTS.index(fmt)
    codes = o._UNPACK[fmt](want[i]).reshape(rows, -1, 32)
    sf = want[3 + i][o.sf_offset(np.arange(rows)[:, None], np.arange(split[i] // 32)[None, :], split[i])]
    mag = codes & ((1 << (f["bits"] - 1)) - 1)
    assert np.all(sf[~big] == 127) and np.all(mag[~big] == 0) and (codes[~big] != 0).any()      # (-0 keeps its sign bit)
    top = (mag == f["maxcode"]) & (np.abs(q) < fmax)
    assert top.any() and np.all(np.abs(q[top]) >= ac.midpoints(fmt)[-1]) and (np.abs(q[top]) > ac.midpoints(fmt)[-1]).any()
    assert col + split[i] <= k


def test_bound_is_the_issue_formula_and_small():
    """the relative bound at x = 0 is (u_exp / 2 + u_rcp + 3 * 2^-24) and stays below 1.5e-6 for |x| <= 8; for x >= 20 it is the three
    roundings and the reciprocal alone"""
    x = o.f32_to_bf16(np.array([0.0, 8.0, -8.0, 20.0, 100.0], np.float32))
    d, a = ac.silu_mul_bound(x, np.full_like(x, 0x3F80))
    k = 1 + 2.0 ** -10
    assert abs(d[0] - (0.5 * ac.U_EXP + ac.U_RCP + 3 * 2.0 ** -24) * k) < 1e-12
    assert d[:3].max() < 1.5e-6 and d[1] < d[2]
    assert abs(d[4] - (ac.U_RCP + 3 * 2.0 ** -24) * k) < 1e-15 and np.all(a == 2.0 ** -149)


@pytest.mark.parametrize("rows,k,split", ac.GAUSSIAN, ids=[f"{c[0]}x{c[1]}" for c in ac.GAUSSIAN])
def test_ambiguous_share_of_the_gaussian_cases_is_under_the_cap(rows, k, split):
    """with the oracle's own scale bytes: the share of elements with more than one admissible code is below the cap, no interval holds
    more than one code boundary, and every code and scale byte of the oracle (numpy's fp32 expf and divide) is admissible"""
    gate, up = ac.gaussian_case(rows, k)
    check_ambiguity(gate, up, rows, split)


def test_ambiguous_share_of_the_all_gate_case():
    gate, up = ac.all_gate_case()
    assert len(np.unique(gate)) == 65536 - 256                      # every finite bf16
    check_ambiguity(gate, up, len(gate), (128, 128, 128))


def check_ambiguity(gate, up, rows, split):
    v = ac.silu_mul_fp64(gate, up)
    assert np.isfinite(v).all()
    d, a = ac.silu_mul_bound(gate, up)
    want = o.activate_quantize(gate, up, *split)
    col, amb, total = 0, 0, 0
    for i, (kseg, fmt) in enumerate(zip(split, ac.FMTS)):
        if not kseg:
            continue
        sl = slice(col, col + kseg)
        col += kseg
        sf = want[3 + i][o.sf_offset(np.arange(rows)[:, None], np.arange(kseg // 32)[None, :], kseg)]
        ok, lo, hi = ac.admissible(v[:, sl], d[:, sl], a[:, sl], sf, fmt)
        codes = o._UNPACK[fmt](want[i]).reshape(rows, kseg)
        plo, phi, pc = ac.code_pos(lo, fmt), ac.code_pos(hi, fmt), ac.code_pos(codes, fmt)
        assert np.all(phi - plo >= 0) and np.all(phi - plo <= 1), fmt
        assert ok.all(), (fmt, "the oracle's own scale bytes are admissible")
        assert np.all((pc >= plo) & (pc <= phi)), (fmt, "the oracle's own codes are admissible")
        amb += int((phi != plo).sum())
        total += lo.size
    assert amb / total < ac.AMBIGUOUS_CAP, amb / total
    return amb / total


@pytest.mark.parametrize("site,m,h,inter,in_split,dsplit", ac.ONEHOT, ids=[c[0] for c in ac.ONEHOT])
def test_onehot_case_is_lossless(site, m, h, inter, in_split, dsplit):
    """x survives reorder_quantize_x with the identity index unchanged, the one-hot weights survive the fp4 weight quantizer, the oracle
    GEMM returns the intended gate / up, every gate is >= 32, and output blocks fall on both sides of the 1e-6 threshold"""
    x, wg, wu, gate, up = ac.onehot_case(m, h, inter)
    ident = np.arange(h, dtype=np.int16)
    qx = o.reorder_quantize(x, ident, *in_split, "x")
    xd = np.concatenate([s for s in o.dequant_operand(qx, "x") if s is not None], axis=1)
    assert np.array_equal(xd, o.bf16_to_f32(x).astype(xd.dtype))
    rows = np.arange(0, inter, max(1, inter // 64))                 # a sample of the weight rows is enough for the GEMM
    for w, want in ((wg, gate), (wu, up)):
        qw = o.reorder_quantize(w[rows], ident, *in_split, "w4")
        wd = np.concatenate([s for s in o.dequant_operand(qw, "w", "w4") if s is not None], axis=1)
        assert np.array_equal(wd, o.bf16_to_f32(w[rows]).astype(wd.dtype))
        assert np.array_equal(o.matmul(*[t for pair in zip(qx[:3], qw[:3]) for t in pair], *[t for pair in zip(qx[3:], qw[3:]) for t in pair]),
                              want[:, rows])
    assert float(o.bf16_to_f32(gate).min()) >= 32.0
    p = exact_product(gate, up)
    assert np.array_equal(o.silu_mul(gate, up).astype(np.float64), p)
    amax = np.abs(p).reshape(m, inter // 32, 32).max(-1)
    assert ((amax > 0) & (amax <= float(ac.F32_1EM6))).any() and (amax > float(ac.F32_1EM6)).mean() > 0.5
