"""Every site that runs the activation quantizer's arithmetic -- v = silu(gate) * up in fp32, quantize32 (csrc/mx_direct_convert.h) --
held to the oracle DIRECTLY, code for code ("Exact-answer activation cases"; tests/act_exact_cases.py has the inputs, the
derivation of the silu_mul bound and the arguments; tests/test_activate_exact_cpu.py proves what they claim without a GPU):

  a. activate_quantize_x (direct_quantize.hip mode 0) on the lossless gate family: every packed byte and every scale byte;
  b. activate_quantize_x on ordinary inputs: every scale byte and every code inside the set the derived bound admits, no share exempt;
  c. down_activate_decode (both in-workgroup quantizers of mx_decode_quant.h) through an identity down_proj;
  d. gate_up_activate / gate_up_activate_decode (mode 3 on the scratch, write_tile_act, the two streaming ACT epilogues) through one-hot
     gate / up weights.
No tolerance here comes from what a kernel produced.  Not covered: the 64-bit r0 / g0 branch of direct_quantize_kernel (it needs 2^31
groups); rmsnorm_gate_up_activate_decode, whose normalisation cannot keep the values lossless -- it stays on its byte-for-byte twin
(tests/test_gate_up_gpu.py), which these tests now anchor."""
import numpy as np
import pytest

import act_exact_cases as ac
from conftest import bits_from_t, t_from_bits, u8
from micromix_amd import _lib, mixedgemm
from oracle import mx_oracle as o

pytestmark = pytest.mark.gpu


def assert_bytes(got, want, rows, split, label, at=None):
    """the six outputs against the oracle's: packed bytes everywhere, scale bytes wherever a row owns them.  `at`: the device rows the
    oracle's rows 0 .. len(at) - 1 stand for (a sample of a larger launch)"""
    at = np.arange(rows) if at is None else np.asarray(at)
    for i in range(3):
        g = u8(got[i])
        assert g.shape == (rows, want[i].shape[1]), (label, i, g.shape)
        g = g[at]
        bad = np.argwhere(g != want[i])
        assert bad.size == 0, f"{label}: packed segment {i}: {len(bad)} bytes differ, first at device row {int(at[bad[0][0]])} byte {int(bad[0][1])}"
        if split[i]:
            j = np.arange(split[i] // 32)[None, :]
            gsf = u8(got[3 + i])[o.sf_offset(at[:, None], j, split[i])]
            wsf = want[3 + i][o.sf_offset(np.arange(len(at))[:, None], j, split[i])]
            bad = np.argwhere(gsf != wsf)
            assert bad.size == 0, (f"{label}: scale bytes of segment {i}: {len(bad)} differ, first at device row {int(at[bad[0][0]])} block "
                                   f"{int(bad[0][1])}: {int(gsf[tuple(bad[0])])} != {int(wsf[tuple(bad[0])])}")


# ---- a ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,k,split", ac.CASES, ids=[f"{c[0]}x{c[1]}" for c in ac.CASES])
def test_activate_quantize_lossless_family(dev, rows, k, split):
    """(37, 128): G = 4 groups per row, a wave's 64 groups span 16 rows and the last step is partial; (130, 1024) holds every edge"""
    gate, up = ac.family(rows, split)
    got = mixedgemm.activate_quantize_x(t_from_bits(gate, dev), t_from_bits(up, dev), *split)
    assert_bytes(got, o.activate_quantize(gate, up, *split), rows, split, f"lossless {rows}x{k}")


def test_activate_quantize_second_trip_of_the_grid_stride_loop(dev):
    """4096 x 8448: 1 081 344 groups, more than the 4096 workgroups x 256 groups of one trip, so rows from 3971 on belong to the second
    trip of direct_quantize_kernel's loop.  The oracle runs on 64 sampled rows from both trips (the family is a function of the row)."""
    rows, k, split = ac.LARGE
    assert rows * k // 32 > ac.TRIP_GROUPS and (rows - 128) * k // 32 <= ac.TRIP_GROUPS      # the smallest such multiple of 128 rows
    gate, up = ac.family(rows, split)
    first2 = ac.TRIP_GROUPS // (k // 32)                  # the row the second trip starts in
    rng = np.random.default_rng(8448)
    at = np.unique(np.concatenate([[0, 1, first2 - 1, first2, first2 + 1, rows - 1], rng.choice(first2, 27, replace=False),
                                   first2 + rng.choice(rows - first2, 31, replace=False)]))
    assert (at < first2).sum() >= 24 and (at > first2).sum() >= 24
    got = mixedgemm.activate_quantize_x(t_from_bits(gate, dev), t_from_bits(up, dev), *split)
    assert_bytes(got, o.activate_quantize(gate[at], up[at], *split), rows, split, "second trip", at=at)


# ---- b ---------------------------------------------------------------------------------------------------------
def check_admissible(dev, gate, up, split, label):
    rows = len(gate)
    got = [u8(t) for t in mixedgemm.activate_quantize_x(t_from_bits(gate, dev), t_from_bits(up, dev), *split)]
    v = ac.silu_mul_fp64(gate, up)
    d, absolute = ac.silu_mul_bound(gate, up)
    col, amb, total = 0, 0, 0
    for i, (kseg, fmt) in enumerate(zip(split, ac.FMTS)):
        if not kseg:
            continue
        sl = slice(col, col + kseg)
        col += kseg
        sf = got[3 + i][o.sf_offset(np.arange(rows)[:, None], np.arange(kseg // 32)[None, :], kseg)]
        ok, lo, hi = ac.admissible(v[:, sl], d[:, sl], absolute[:, sl], sf, fmt)
        assert ok.all(), f"{label} {fmt}: {int((~ok).sum())} scale bytes outside the exponent rule of every admissible amax, first {np.argwhere(~ok)[0]}"
        pc = ac.code_pos(o._UNPACK[fmt](got[i]).reshape(rows, kseg), fmt)
        plo, phi = ac.code_pos(lo, fmt), ac.code_pos(hi, fmt)
        bad = (pc < plo) | (pc > phi)
        assert not bad.any(), f"{label} {fmt}: {int(bad.sum())} codes outside the admissible set, first at {np.argwhere(bad)[0]}"
        amb += int((phi != plo).sum())
        total += pc.size
    print(f"{label}: {amb} of {total} elements have two admissible codes ({amb / total:.2e})")
    assert amb / total < ac.AMBIGUOUS_CAP, (label, amb / total)        # the check is not vacuous (proved on the CPU as well)


@pytest.mark.parametrize("rows,k,split", ac.GAUSSIAN, ids=[f"{c[0]}x{c[1]}" for c in ac.GAUSSIAN])
def test_activate_quantize_admissible_codes_gaussian(dev, rows, k, split):
    """the inputs of test_direct_quantize_gpu.py::test_activate_quantize_close_to_oracle: every scale byte is the exponent rule of an
    amax within the derived silu_mul bound of the fp64 amax, and every code -- at the scale byte the device wrote -- the RNE code of a
    value within the bound of the fp64 value"""
    gate, up = ac.gaussian_case(rows, k)
    check_admissible(dev, gate, up, split, f"gaussian {rows}x{k}")


def test_activate_quantize_admissible_codes_every_gate(dev):
    """the gate columns run over every finite bf16: the exp2 overflow and rcp flush ranges, denormal gates, gates past +-8"""
    gate, up = ac.all_gate_case()
    check_admissible(dev, gate, up, (128, 128, 128), "every gate")


# ---- c ---------------------------------------------------------------------------------------------------------
# (M, I, split): each format, alone and mixed; 4 x 4224 / 32 = 528 groups > 512 threads: two passes of activate_rows_to_lds, where the
# others take the one-pass activate_rows_early
DOWN = [(1, 512, (512, 0, 0)), (4, 512, (0, 512, 0)), (1, 512, (0, 0, 512)), (4, 1280, (512, 384, 384)), (1, 1280, (1024, 128, 128)),
        (4, 4224, (2048, 1024, 1152))]


@pytest.mark.parametrize("wmode", ("w4", "w"))
@pytest.mark.parametrize("m,inter,split", DOWN, ids=[f"{c[0]}x{c[1]}x{'-'.join(map(str, c[2]))}" for c in DOWN])
def test_down_activate_decode_identity_down_proj(dev, m, inter, split, wmode):
    """down_proj = the bf16 identity [I, I]: its codes are 1.0 exactly (fp4 4 * 2^-2, fp6 16 * 2^-4, fp8 256 * 2^-8) and every other
    block is empty, so D[m, n] is the single product dequant(h)[m, n] * 1.0 -- a code value times a power of two, which fits bf16 --
    plus zeros.  D therefore shows the codes AND scales the in-workgroup quantizer produced: bit-equal to the dequantised
    o.activate_quantize of the lossless family.  Not visible here: the scale byte of a block whose codes are all zero (127 or anything
    else gives 0), and the sign of a zero (0 + -0 = +0); part a sees both."""
    import torch
    gate, up = ac.family(m, split, seed=inter + m)
    eye = torch.eye(inter, dtype=torch.bfloat16, device=dev)
    b = (mixedgemm.downproj_quantize_w4 if wmode == "w4" else mixedgemm.downproj_quantize_w)(eye, *split)
    assert mixedgemm.down_activate_decode_supported(m, inter, *split) >= 1
    gu = t_from_bits(ac.interleave(gate, up), dev)
    want6 = o.activate_quantize(gate, up, *split)
    want = np.concatenate([o.dequant_segment(want6[i], want6[3 + i], m, split[i], ac.FMTS[i]) for i in range(3)], axis=1)
    wbits = o.f32_to_bf16(want + np.float32(0))                               # (-0 -> +0)
    assert np.array_equal(o.bf16_to_f32(wbits), want) and (want != 0).mean() > 0.3       # fits bf16; most outputs are live
    for rounding in ("reference", "fused"):
        got = bits_from_t(mixedgemm.down_activate_decode(gu, b, *split, rounding=rounding))
        bad = np.argwhere(got != wbits)
        assert bad.size == 0, (rounding, len(bad), bad[:4].tolist(), [(hex(int(got[tuple(p)])), hex(int(wbits[tuple(p)]))) for p in bad[:4]])


# ---- d ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("site,m,h,inter,in_split,dsplit", ac.ONEHOT, ids=[c[0] for c in ac.ONEHOT])
def test_gate_up_activate_one_hot_weights(dev, site, m, h, inter, in_split, dsplit):
    """one-hot gate / up weights copy chosen activation values (gate >= 32) into gate and up inside the fused launch: its six outputs
    equal o.activate_quantize of the INTENDED gate and up, byte for byte, at every site -- the quantizer on the interleaved scratch
    (M <= 64), write_tile_act (M > 64), the streaming ACT epilogue with one token tile (M <= 16) and with two (17 .. 32)"""
    import torch
    x, wg, wu, gate, up = ac.onehot_case(m, h, inter)
    desc = _lib.load().mm_gate_up_activate_describe(m, inter).decode()
    if site.startswith("stream"):
        if 2 * inter // 64 < torch.cuda.get_device_properties(dev).multi_processor_count:
            pytest.fail(f"the layer is not wide on this device ({desc}): choose I for its CU count")
        assert "stream_act" in desc, desc
    else:
        assert "stream_act" not in desc and ("act_kernel" in desc) == (site == "tile") and ("direct_quantize_kernel<0,true>" in desc) == (site == "scratch"), desc
    idx = torch.arange(h, dtype=torch.int16, device=dev)
    xt = t_from_bits(x, dev)
    qx = mixedgemm.reorder_quantize_x(xt, idx, *in_split)
    want_x = o.reorder_quantize(x, np.arange(h, dtype=np.int16), *in_split, "x")
    assert all(np.array_equal(u8(qx[i]), want_x[i]) for i in range(3))
    qgu = mixedgemm.interleave_gate_up(mixedgemm.reorder_quantize_w4(t_from_bits(wg, dev), idx, *in_split),
                                       mixedgemm.reorder_quantize_w4(t_from_bits(wu, dev), idx, *in_split))
    want = o.activate_quantize(gate, up, *dsplit)
    for rounding in ("reference", "fused"):
        assert_bytes(mixedgemm.gate_up_activate(qx, qgu, *dsplit, rounding=rounding), want, m, dsplit, f"{site} {rounding}")
        if m <= 4:
            assert mixedgemm.gate_up_activate_decode_supported(m, inter, *in_split) >= 1
            assert_bytes(mixedgemm.gate_up_activate_decode(xt, idx, qgu, *dsplit, rounding=rounding), want, m, dsplit, f"{site} bf16 rows {rounding}")
