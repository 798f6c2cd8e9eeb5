"""GPU tests that pin the oracle and the kernel's layout assumptions against the CDNA4 hardware:
the scaled-MFMA operand / scale / accumulator register layouts, and AMD's own MX converter
instructions (an independent implementation of the OCP encodings)."""
import numpy as np
import pytest

import hw_layout as hl
from conftest import t_from_bits
from micromix_amd import _lib
from oracle import mx_oracle as o

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", (32, 16))
@pytest.mark.parametrize("el_a", hl.ELS)
@pytest.mark.parametrize("el_b", hl.ELS)
def test_scaled_mfma_register_layout(dev, shape, el_a, el_b):
    import torch
    lib = _lib.load_diag()
    rng = np.random.default_rng(shape * 100 + hl.ELS.index(el_a) * 10 + hl.ELS.index(el_b))
    # fp4 x fp4 / fp4 x fp6 products are summed exactly by the hardware; anything with fp8 or
    # fp6 x fp6 goes through a limited-precision adder tree (documented in tests/gemm_check.py)
    exact = {el_a, el_b} <= {"fp4", "fp6"} and (el_a, el_b) != ("fp6", "fp6")
    tol = 1e-6 if exact else 5e-4
    for opsel in range(4):
        for _ in range(3):
            err, _, _ = hl.run_case(lib, torch, dev, rng, shape, el_a, el_b, opsel)
            assert err < tol, (shape, el_a, el_b, opsel, err)


@pytest.mark.parametrize("el", hl.ELS)
def test_oracle_encoders_match_hardware_converters(dev, el):
    """v_cvt_scalef32_pk_{fp4,fp8}_bf16 / v_cvt_scalef32_pk32_bf6_bf16 (dst = cvt(src / scale)) produce
    exactly the oracle's codes for every finite bf16 whose scaled value is in range."""
    import torch
    lib = _lib.load_diag()
    allb = np.arange(65536, dtype=np.uint16)
    src = allb[np.isfinite(o.bf16_to_f32(allb))]
    src = src[: len(src) // 32 * 32]
    tsrc = t_from_bits(src, dev)
    x = o.bf16_to_f32(src).astype(np.float64)
    fm = o.FORMATS[el]["fmax"]
    # -127: the scale operand is read as E8M0 (exponent field only), so the bit pattern 0 -- and any fp32 denormal -- means 2^-127;
    # the quantizers rely on it for blocks whose absmax is below FMAX * 2^-127 (mx_group_convert.h: convert_group)
    for e, scale in ((-20, None), (-3, None), (0, None), (2, None), (17, None), (-127, 0.0), (-127, 2.0 ** -127), (-127, 2.0 ** -130)):
        out = torch.zeros(len(src), dtype=torch.uint8, device=dev)
        assert lib.mm_diag_hw_convert(tsrc.data_ptr(), len(src), float(2.0 ** e) if scale is None else scale, hl.ELS.index(el), out.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        scaled = x / 2.0 ** e
        inr = np.abs(scaled) <= fm
        want = o.encode(np.clip(scaled, -2 * fm, 2 * fm).astype(np.float32), el)
        got = out.cpu().numpy()
        assert inr.sum() > (1000 if e > -127 else 500) and np.array_equal(got[inr], want[inr]), (el, e, scale)


F32_SCALES = (-20, -3, 0, 2, 17)


def f32_converter_inputs(el, past_fmax=False):
    """fp32 values in units of the scale, all different: every midpoint between adjacent codes (the first is half the smallest subnormal),
    FMAX, each with the fp32 on either side; 0; more than 100 000 random values with full 24-bit significands from below the smallest
    subnormal up to FMAX; all of them in both signs, shuffled so that the 32 positions of every group hold different values.
    `past_fmax`: the values beyond FMAX instead -- a few fixed ones up to 2^30 FMAX and random ones up to 4 FMAX"""
    import act_exact_cases as ac
    fm = o.FORMATS[el]["fmax"]
    rng = np.random.default_rng(32 + hl.ELS.index(el) + (100 if past_fmax else 0))
    edge = np.concatenate([ac.midpoints(el), [fm]]).astype(np.float32)
    assert np.array_equal(edge.astype(np.float64), np.concatenate([ac.midpoints(el), [fm]]))        # short values: exact in fp32
    edge = np.concatenate([edge, np.nextafter(edge, np.float32(0)), np.nextafter(edge, np.float32(np.inf)), [np.float32(0)]])
    past = np.array([1.0625, 1.5, 2, 3.999, 1000, 2.0 ** 30], np.float32) * np.float32(fm)
    smin = float(ac.midpoints(el)[0]) * 2
    lo, hi = (int(np.log2(fm)), int(np.log2(fm)) + 2) if past_fmax else (int(np.log2(smin)) - 3, int(np.log2(fm)))
    sig = (rng.integers(1 << 23, 1 << 24, size=2_000 if past_fmax else 140_000) | 1).astype(np.float64)    # bit 0 set: 24 significant bits
    rnd = (sig * np.exp2(rng.integers(lo, hi + 1, size=sig.size) - 23.0)).astype(np.float32)
    rnd = rnd[(rnd > np.nextafter(np.float32(fm), np.float32(np.inf))) & (rnd < 4 * fm)] if past_fmax else rnd[rnd < fm]
    keep = np.unique(past if past_fmax else edge)
    rnd = np.setdiff1d(rnd, keep)
    rnd = rnd[: len(rnd) - (len(rnd) + len(keep)) % 16]                                            # whole groups of 32 once both signs are in
    pos = np.concatenate([keep, rnd])
    x = np.concatenate([pos, -pos])                                                                # (+0 and -0 are both in it)
    x = x[rng.permutation(len(x))]
    assert len(x) % 32 == 0 and len(rnd) >= (500 if past_fmax else 100_000) and np.isin(np.concatenate([keep, -keep]), x).all()
    g = np.sort(x.view(np.uint32).reshape(-1, 32), axis=1)
    assert np.all(g[:, 1:] != g[:, :-1])                                                           # 32 different bit patterns per group
    return x


def hw_convert_f32(dev, el, x, scale, saturate):
    import torch
    src = torch.from_numpy(x).to(dev)
    out = torch.full((len(x),), 0xEE, dtype=torch.uint8, device=dev)
    assert _lib.load_diag().mm_diag_hw_convert_f32(src.data_ptr(), len(x), float(scale), hl.ELS.index(el), int(saturate), out.data_ptr(),
                                                   torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_f32_converter(dev, el, u, saturate, want=None):
    want = o.encode(u, el) if want is None else want
    for e in F32_SCALES:
        x = (u.astype(np.float64) * 2.0 ** e).astype(np.float32)
        assert np.array_equal(np.float32(x.astype(np.float64) / 2.0 ** e).view(np.uint32), u.view(np.uint32))   # the scaling is exact
        got = hw_convert_f32(dev, el, x, 2.0 ** e, saturate)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (el, e, saturate, f"{bad.size} of {len(u)} codes differ; (x / scale, got, want, position): ",
                               [(float(u[i]), int(got[i]), int(want[i]), int(i % 32)) for i in bad[:8]])
    return want


@pytest.mark.parametrize("el", hl.ELS)
def test_f32_converters(dev, el):
    """v_cvt_scalef32_pk_{fp4,fp8}_f32 / v_cvt_scalef32_2xpk16_bf6_f32 through the quantizers' own convert32 (csrc/mx_direct_convert.h:
    its converter calls, its MM_BF6_LO / MM_BF6_HI element order, its packing), unclamped exactly as quantize32 calls it and in its
    saturating form: exactly the oracle's code for every input up to FMAX (and the fp32 next above it), one rounding from fp32 -- ties
    to even, the fp32 next to a tie on its own side, the sign kept on zero -- at scales 2^-20 .. 2^17.  Every position of a group holds
    a different value, so an element-order error changes codes."""
    u = f32_converter_inputs(el)
    want = check_f32_converter(dev, el, u, saturate=0)
    check_f32_converter(dev, el, u, saturate=1)
    assert len(np.unique(want)) == 2 * o.FORMATS[el]["maxcode"] + 2          # every code of the format, both zeros
    assert _lib.load_diag().mm_diag_hw_convert_f32(None, 33, 1.0, 0, 1, None, None) == _lib.MM_ERR_BAD_ARG


@pytest.mark.parametrize("el", hl.ELS)
def test_f32_converters_past_fmax(dev, el):
    """|x / scale| > FMAX.  convert32's saturating form (what a caller with a scale of its own takes) gives the oracle's satfinite code,
    +-FMAX, in every format.  The bare converters -- what quantize32 runs, whose exponent rule keeps amax / scale <= FMAX for every
    finite block -- are pinned as the hardware fact they are: fp4 and fp6 saturate by themselves; v_cvt_scalef32_pk_fp8_f32 rounds to
    nearest even without saturating, so below 464 (the midpoint to the absent 480) it gives 448 and above it the e4m3 NaN code 0x7F / 0xFF
    (first measured on an MI355X: 468.5 -> 0x7F, -557.6 -> 0xFF, 981.3 -> 0x7F).  If a later part saturates here, SAT can go."""
    u = f32_converter_inputs(el, past_fmax=True)
    check_f32_converter(dev, el, u, saturate=1)
    bare = o.encode(u, el)
    if el == "fp8":
        assert (np.abs(u) < 464).sum() > 50 and (np.abs(u) > 464).sum() > 1000 and not (np.abs(u) == 464).any()
        bare = np.where(np.abs(u) > 464, bare | 0x7F, bare).astype(np.uint8)
    check_f32_converter(dev, el, u, saturate=0, want=bare)


SILU_B = (0x3F80, 0xBF80, 0x3FFF, 0xBF4D, 0x40D5, 0x3EAB)        # 1, -1, 1.9921875, -0.80078125, 6.65625, 0.333984375


def test_silu_mul_against_fp64(dev):
    """silu_mul (csrc/mx_direct_convert.h: hardware exp2 and rcp) for EVERY finite bf16 gate against x / (1 + e^-x) * b in fp64, within
    the bound derived in tests/act_exact_cases.py from the documented accuracy of v_exp_f32 / v_rcp_f32 (nothing fitted); in the
    flush ranges (exp2 overflow, rcp result below 2^-126) between the value and the zero of its sign; and for every gate >= 20 the exact
    product a * b, bit for bit -- what the lossless family of tests/test_activate_exact_gpu.py rests on.
    Measured on an MI355X: see DESIGN.md, "Exact-answer activation cases"."""
    import torch
    import act_exact_cases as ac
    lib = _lib.load_diag()
    allb = np.arange(65536, dtype=np.uint16)
    fin = allb[np.isfinite(o.bf16_to_f32(allb))]
    a = np.tile(fin, len(SILU_B))
    b = np.repeat(np.array(SILU_B, np.uint16), len(fin))
    out = torch.full((len(a),), float("nan"), dtype=torch.float32, device=dev)
    assert lib.mm_diag_silu_mul(t_from_bits(a, dev).data_ptr(), t_from_bits(b, dev).data_ptr(), len(a), out.data_ptr(),
                                torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    x = o.bf16_to_f32(a).astype(np.float64)
    v = ac.silu_mul_fp64(a, b)
    d, absolute = ac.silu_mul_bound(a, b)
    ok = np.isfinite(v)                                          # (|a * b| past fp32: inf is out of scope)
    ok &= np.abs(v) < 2.0 ** 127
    err = np.abs(got.astype(np.float64) - v)
    normal = ok & (np.abs(v) >= 2.0 ** -126) & (x * -ac.LOG2E < 125.5)
    ulps = err[normal] / np.exp2(np.floor(np.log2(np.abs(v[normal]))) - 23)
    worst = int(np.argmax(np.where(normal, err / np.maximum(d * np.abs(v) + absolute, 1e-300), 0)))
    near = np.abs(x[normal]) <= 8
    print(f"silu_mul: max error {ulps[near].max():.3f} fp32 ulps over |gate| <= 8, {ulps.max():.3f} over every gate (the error of t grows with |t|), max error / bound {float(err[worst] / (d[worst] * abs(v[worst]) + absolute[worst])):.3f} "
          f"at gate {x[worst]!r} b {float(o.bf16_to_f32(b[worst:worst + 1])[0])!r}; max relative error {float((err[normal] / np.abs(v[normal])).max()):.3e}")
    assert np.all(np.isfinite(got[ok]))
    assert np.array_equal(np.signbit(got[ok]), np.signbit(v[ok]))
    over = ok & (err > d * np.abs(v) + absolute)
    assert not over.any(), (int(over.sum()), [(float(x[i]), float(got[i]), float(v[i])) for i in np.flatnonzero(over)[:8]])
    lossless = ok & (x >= ac.GATE_MIN)
    with np.errstate(over="ignore"):                            # (products past fp32 are not `ok`)
        exact = (x * o.bf16_to_f32(b).astype(np.float64)).astype(np.float32)
    assert lossless.sum() > 6 * 6000 and np.array_equal(got[lossless].view(np.uint32), exact[lossless].view(np.uint32))
