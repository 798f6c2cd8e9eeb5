"""The preconditions of tests/test_gemm_exact_gpu.py, proved without a GPU for every case that file runs (its `all_cases()`):

  * the packing is lossless: o.dequant_operand of the packed operands is the intended values, both weight modes;
  * fp32 arithmetic on them is exact in any order: |running value| + sum_k |x||w|, counted in units of the smallest product bit, stays
    below 2^24 -- from the data, per output, up to FULL outputs; from the operands (Cauchy-Schwarz, a larger figure) above that;
  * the expected bits are o.matmul's on the packed operands, both rounding modes and with bias, up to FULL outputs: the oracle and the
    closed-form answer are the same thing;
  * the data covers what it claims: every exponent value in every 128-deep slab of every ROW (hence of every row tile and every
    16-row group), every element code the recipe can produce, no two rows alike, and outputs with exact bf16 ties, both signs and
    exact zeros;
  * a kernel that took one block's scale from the next block, dropped a 128-deep slab or swapped two rows of a tile would change at
    least 90 % of the outputs it touches.

Where a property is asserted per case only above a size, the size is reasoned: an alphabet of 8 values (7 and the pin) is complete in
a segment of 4096 elements except with probability 8 * (6/7)^4096; a sum of K products of standard deviation s hits one given multiple
of 0.5 with probability about 0.2 / s (s < 1300 for K <= 2560), so 2^17 outputs hold more than 20 exact zeros on average; ties need an
output of at least 128 with an odd number of halves, which half of those outputs have."""
import numpy as np
import pytest

import gemm_exact_cases as gx
from oracle import mx_oracle as o
from test_gemm_exact_gpu import all_cases

FULL = 1 << 22          # outputs up to which a case's products are formed here
CASES = sorted(set(all_cases()))
_codes_seen = {}


def _mm(q, w, rounding, wdeq):
    return o.matmul(q[0], w[0], q[1], w[1], q[2], w[2], q[3], w[3], q[4], w[4], q[5], w[5], rounding=rounding, b_dequant=wdeq)


def _ties(f32):
    """outputs that lie exactly half way between two bf16 values"""
    return (np.ascontiguousarray(f32, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF)) == np.uint32(0x8000)


def _alphabet_codes(kind, fmt):
    vals, pin = (np.arange(-3, 4, dtype=np.float32), gx.X_PIN) if kind == "x" else (np.arange(-2, 3, dtype=np.float32) * 0.5, gx.W_PIN)
    e0 = int(o.scale_exponent(np.array([pin], np.float32), fmt)[0])
    return set(o.encode(np.append(vals, np.float32(pin)) * np.float32(2.0 ** -e0), fmt).tolist())


def _seen(q, kind, fmts, split):
    unpack = {"fp4": o.unpack_fp4, "fp6": o.unpack_fp6, "fp8": lambda b: b}
    for i, (fmt, kseg) in enumerate(zip(fmts, split)):
        if kseg and q[i].size:
            codes = set(np.flatnonzero(np.bincount(unpack[fmt](q[i]).ravel(), minlength=256)).tolist())
            assert codes <= _alphabet_codes(kind, fmt)
            _codes_seen.setdefault((kind, fmt), set()).update(codes)
            if q[i].shape[0] * kseg >= 4096:
                assert codes == _alphabet_codes(kind, fmt), (kind, fmt, sorted(codes))


@pytest.mark.parametrize("M,N,split,seed,wmodes", CASES, ids=[f"{c[0]}x{c[1]}-{'_'.join(map(str, c[2]))}-{'+'.join(c[4])}" for c in CASES])
def test_preconditions(M, N, split, seed, wmodes):
    assert all(gx.RANGES[w] == gx.RANGES["w4"] for w in wmodes)              # one set of intended values serves both modes
    v = gx.exact_values(M, N, split, seed)
    qx = gx.pack(v, "x")
    gx.assert_lossless(qx, v, "x")
    _seen(qx, "x", gx.X_FMTS, split)
    qws, wdeq = {}, {}
    for wmode in wmodes:
        qws[wmode] = gx.pack(v, "w", wmode)
        wdeq[wmode] = gx.assert_lossless(qws[wmode], v, "w", wmode)
        _seen(qws[wmode], "w", gx.w_formats(wmode), split)
    # coverage of the exponents and of the rows
    col = 0
    for i, kseg in enumerate(split):
        for exp, n in ((v.xexp, gx.RANGES["w4"][i][0]), (v.wexp, gx.RANGES["w4"][i][1])):
            e = exp[:, col // 32:(col + kseg) // 32].reshape(exp.shape[0], kseg // 128, 4)
            assert e.size == 0 or (np.sort(np.unique(e)) == np.arange(n)).all()
            assert all((e == val).any(axis=2).all() for val in range(n)), "an exponent value is missing from a slab of a row"
            assert (e[..., 1:] != e[..., :-1]).all(), "two neighbouring blocks of a slab share their exponent"
        col += kseg
    for base, exp in ((v.xbase, v.xexp), (v.wbase, v.wexp)):
        rows = np.ascontiguousarray(np.concatenate([base, exp], axis=1))
        assert len({r.tobytes() for r in rows}) == len(rows), "two rows carry identical data"
    if M == 0:
        return
    # exactness of fp32 sums in any order
    full = M * N <= FULL
    parts = gx.segment_products(v) if full else None
    units = gx.exactness_units(v, parts)
    assert units < 2 ** 24, units
    if not full:
        return
    assert gx.exactness_units(v) >= units                                       # the operand-only figure used above FULL is a bound
    want = gx.rounding_chain(parts, v.bias, M, N)
    for wmode in wmodes:
        for rounding in ("reference", "fused"):
            got = _mm(qx, qws[wmode], rounding, wdeq[wmode])
            assert np.array_equal(got, want[rounding]), (wmode, rounding)
            with_bias = o.f32_to_bf16(o.bf16_to_f32(got) + v.bias[None, :])      # qlinear_forward's bias step
            assert np.array_equal(with_bias, want[rounding + "+bias"]), (wmode, rounding, "bias")
    f32 = want["f32"]
    if M * N >= 1024:
        assert (f32 > 0).any() and (f32 < 0).any() and _ties(f32).any()
        y = o.bf16_to_f32(want["reference"]) + v.bias[None, :]
        assert _ties(y).any() and (~_ties(y)).any(), "the bias step needs both exact ties and non-ties"
    if M * N >= 1 << 17 and sum(split) <= 2560:
        assert (f32 == 0).any() and (want["fused"] == 0).any()


def test_every_code_is_produced():
    """every fp4, fp6 and fp8 code the recipe can produce, in both operands (test_preconditions asserts the same of every segment of
    4096 elements or more of every case)"""
    v = gx.exact_values(300, 520, (256, 128, 256), 2)
    _codes_seen.clear()
    _seen(gx.pack(v, "x"), "x", gx.X_FMTS, v.split)
    _seen(gx.pack(v, "w", "w"), "w", gx.X_FMTS, v.split)
    for kind in ("x", "w"):
        for fmt in gx.X_FMTS:
            assert _codes_seen[(kind, fmt)] == _alphabet_codes(kind, fmt), (kind, fmt)
    assert len(_alphabet_codes("x", "fp8")) == 8 and len(_alphabet_codes("w", "fp4")) == 6


def test_packing_is_what_the_quantizer_writes():
    """the closed-form bytes are the bytes o.reorder_quantize gives the intended values under any reorder index"""
    rng = np.random.default_rng(3)
    M, N, split = 70, 130, (256, 128, 256)
    K = sum(split)
    v = gx.exact_values(M, N, split, 5)
    idx = rng.permutation(K).astype(np.int16)
    inv = np.argsort(idx)
    for kind, modes in (("x", ("x",)), ("w", ("w", "w4"))):
        vals = np.concatenate(gx.segments(v, kind), axis=1).astype(np.float32)
        bits = o.f32_to_bf16(vals)
        assert np.array_equal(o.bf16_to_f32(bits), vals)
        for mode in modes:
            want = o.reorder_quantize(bits[:, inv], idx, *split, mode)           # column idx[j] of the source is reordered column j
            got = gx.pack(v, kind, mode)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), (kind, mode)


def test_product_backends_agree():
    """numpy fp64, torch fp64 and integer arithmetic give the same product (the GPU file runs it with torch on the device)"""
    import torch
    v = gx.exact_values(96, 160, (128, 128, 128), 9)
    for x, w in zip(gx.segments(v, "x"), gx.segments(v, "w")):
        exact = (x.astype(np.int64) @ (2 * w).astype(np.int64).T) / 2.0
        assert np.array_equal((2 * w).astype(np.int64), 2 * w) and np.array_equal(x.astype(np.int64), x)
        assert np.array_equal(gx.product(x, w), exact) and np.array_equal(gx.product(x, w, torch.device("cpu")), exact)


@pytest.mark.parametrize("M,N,split", [(96, 160, (128, 128, 128)), (300, 520, (256, 128, 256)), (40, 264, (0, 0, 1024))])
def test_sensitivity(M, N, split):
    """what a subtly wrong kernel would compute differs from the expected output on at least 90 % of the outputs it touches, in the
    rounded output as well as in the fp32 one"""
    v = gx.exact_values(M, N, split, 21)
    xs, ws = gx.segments(v, "x"), gx.segments(v, "w")
    present = [i for i, k in enumerate(split) if k]
    want = gx.rounding_chain([xs[i] @ ws[i].T for i in present], v.bias, M, N)

    def changed(xs2, ws2, rows=slice(None)):
        got = gx.rounding_chain([xs2[i] @ ws2[i].T for i in present], v.bias, M, N)
        return min(float((got[k][rows] != want[k][rows]).mean()) for k in ("reference", "fused", "f32"))

    col = 0
    for i in present:
        nblk = split[i] // 32
        for kind in ("x", "w"):
            exp = (v.xexp if kind == "x" else v.wexp)[:, col // 32:col // 32 + nblk].astype(np.float64)
            for b in (0, 1, 2, nblk - 2):                    # one block's scale taken from the next block of its slab
                ops = [list(xs), list(ws)]
                seg = ops[kind == "w"][i].copy().reshape(-1, nblk, 32)
                seg[:, b] *= np.exp2(exp[:, b + 1] - exp[:, b])[:, None]
                ops[kind == "w"][i] = seg.reshape(-1, split[i])
                assert changed(*ops) >= 0.9, (i, kind, b, changed(*ops))
        for slab in range(split[i] // 128):                   # one 128-deep slab dropped
            x2 = list(xs)
            x2[i] = xs[i].copy()
            x2[i][:, 128 * slab:128 * slab + 128] = 0
            assert changed(x2, ws) >= 0.9, (i, slab, changed(x2, ws))
        col += split[i]
    for r0, r1 in ((0, 1), (3, 19), (15, 16), (M - 1, M // 2)):  # two rows of a tile swapped (neighbours, across and inside 16-row groups)
        x2 = [None if x is None else x.copy() for x in xs]
        for x, src in zip(x2, xs):
            if x is not None:
                x[[r0, r1]] = src[[r1, r0]]
        assert changed(x2, ws, rows=[r0, r1]) >= 0.9, (r0, r1, changed(x2, ws, rows=[r0, r1]))
