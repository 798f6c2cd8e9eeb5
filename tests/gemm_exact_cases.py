"""GEMM inputs whose answer is known exactly, for tests/test_gemm_exact_cpu.py and tests/test_gemm_exact_gpu.py.

The recipe ("Exact-answer GEMM cases").  In reordered order -- there is no reorder index, the operands are built packed --
every 32-block of an activation row holds integers in -3..3 and one element pinned to 6; every block of a weight row holds values in
{-1, -0.5, 0, 0.5, 1} and one element pinned to 3.  The pinned position is a hash of (row, block), different for the two operands, so
the two pins meet in about one block of 32.  Block b of activation row m is then multiplied by 2^sx(m, b) and block b of weight row n by
2^sw(n, b): inside every 128-deep slab (four blocks) of every row the exponents are an arrangement, chosen by a hash of (row, slab), in
which every value of the range occurs and no two neighbouring blocks are equal.  A kernel that takes a scale from the block next door,
from another row or from another slab therefore changes the sums.

Every such value is a code of fp4, fp6 and fp8 at the block scale the project's quantizer would choose (the pin is the block's amax), so
the packed bytes are written in closed form with the oracle's encoders and `sf_offset`; `assert_lossless` proves it with
`o.dequant_operand`.  Every product is a multiple of 0.5 and every partial sum stays far below 2^24 of those units (`exactness_units`),
so fp32 accumulation in any order, split over any number of waves or launches, gives the same bits: the expected output is the fp64
product of the INTENDED values -- never of the packed bytes -- put through the project's rounding chain with `o.f32_to_bf16`.

All data is a pure function of (row, column, seed): the first rows of a larger case are the rows of a smaller one."""
import itertools
from collections import namedtuple

import numpy as np

from oracle import mx_oracle as o

X_PIN, W_PIN = 6.0, 3.0
X_FMTS = ("fp4", "fp6", "fp8")
_PACK = {"fp4": o.pack_fp4, "fp6": o.pack_fp6, "fp8": lambda c: np.asarray(c, dtype=np.uint8)}

# Exponent ranges per segment, (number of sx values, number of sw values): sx in 0..3 and sw in 0..2.  Measured on the MI355X
# (DESIGN.md): every format pair sums these blocks exactly when the four blocks of a 128-deep MFMA carry different exponents, so no
# pair needs a narrower range.  An entry may be narrowed to (2, 2), or set to "row" (one exponent per row, 0..3 / 0..2, the same for
# all its blocks), per weight mode and segment.
RANGES = {"w4": ((4, 3), (4, 3), (4, 3)), "w": ((4, 3), (4, 3), (4, 3))}

_MASK = (1 << 64) - 1


def w_formats(wmode):
    return ("fp4", "fp4", "fp4") if wmode == "w4" else X_FMTS


def _hash(a, b, salt):
    """splitmix64 finaliser over (a, b, salt), vectorised; a and b broadcast"""
    s = np.uint64((salt * 0xD6E8FEB86659FD93 + 0x2545F4914F6CDD1D) & _MASK)
    h = (np.asarray(a, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ (np.asarray(b, dtype=np.uint64) * np.uint64(0xC2B2AE3D27D4EB4F)) ^ s
    h = (h ^ (h >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    h = (h ^ (h >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return h ^ (h >> np.uint64(31))


def arrangements(nvals):
    """every way to give the four blocks of a slab exponents 0..nvals-1 such that each value occurs and neighbours differ"""
    return np.array([a for a in itertools.product(range(nvals), repeat=4)
                     if len(set(a)) == nvals and all(a[i] != a[i + 1] for i in range(3))], dtype=np.int8)


def _exponents(rows, kseg, col0, rng_spec, salt):
    """[rows, kseg / 32] block exponents"""
    nslab = kseg // 128
    r = np.arange(rows, dtype=np.int64)[:, None]
    if rng_spec[0] == "row":
        e = (_hash(r, 0, salt) % np.uint64(rng_spec[1])).astype(np.int8)
        return np.broadcast_to(e, (rows, nslab * 4)).copy()
    arr = arrangements(rng_spec[1])
    slab = (col0 // 128 + np.arange(nslab, dtype=np.int64))[None, :]
    pick = (_hash(r, slab, salt) % np.uint64(len(arr))).astype(np.int64)
    return arr[pick].reshape(rows, nslab * 4)


def _operand(rows, split, seed, kind, ranges):
    """(base values int8 [rows, K] in units of 1 (x) or 0.5 (w), block exponents int8 [rows, K / 32]) of one operand"""
    K = sum(split)
    r = np.arange(rows, dtype=np.int64)[:, None]
    h = _hash(r, np.arange(K, dtype=np.int64)[None, :], 4 * seed + (0 if kind == "x" else 1))
    base = ((h % np.uint64(7)).astype(np.int8) - 3) if kind == "x" else ((h % np.uint64(5)).astype(np.int8) - 2)
    pin = (_hash(r, np.arange(K // 32, dtype=np.int64)[None, :], 4 * seed + (2 if kind == "x" else 3)) % np.uint64(32)).astype(np.int64)
    if rows and K:
        np.put_along_axis(base.reshape(rows, K // 32, 32), pin[..., None], 6, axis=2)     # 6 = X_PIN, and W_PIN in units of 0.5
    exps, col0 = [], 0
    for i, kseg in enumerate(split):
        spec = ranges[i]
        n = spec[0 if kind == "x" else 1] if spec != "row" else None
        spec = ("row", 4 if kind == "x" else 3) if n is None else ("block", n)
        exps.append(_exponents(rows, kseg, col0, spec, 64 * seed + 8 * i + (5 if kind == "x" else 6)))
        col0 += kseg
    return base, (np.concatenate(exps, axis=1) if K else np.zeros((rows, 0), np.int8))


class Values(namedtuple("Values", "M N split seed ranges xbase xexp wbase wexp bias cache")):
    """the intended operands: base values and block exponents (`segments` turns them into fp64 values, once per operand)"""
    __slots__ = ()


def exact_values(M, N, split, seed, ranges=None):
    """the intended operands (independent of the weight mode when the two modes share their ranges) and the bias (float32 [N])"""
    ranges = tuple(ranges) if ranges is not None else RANGES["w4"]
    xbase, xexp = _operand(M, split, seed, "x", ranges)
    wbase, wexp = _operand(N, split, seed, "w", ranges)
    bias = ((_hash(np.arange(N, dtype=np.int64), 0, 4 * seed + 7) % np.uint64(13)).astype(np.float32) - 6) * 0.5   # -3 .. 3 in halves
    return Values(M, N, tuple(split), seed, ranges, xbase, xexp, wbase, wexp, bias, {})


def segments(v, kind):
    """the three segments of an operand's intended values as fp64 [rows, Kseg] (None where empty), as o.dequant_operand returns them"""
    if kind in v.cache:
        return v.cache[kind]
    base, exp, unit = (v.xbase, v.xexp, 1.0) if kind == "x" else (v.wbase, v.wexp, 0.5)
    out, col = v.cache.setdefault(kind, []), 0
    for kseg in v.split:
        if kseg == 0:
            out.append(None)
            continue
        b = base[:, col:col + kseg].astype(np.float64).reshape(-1, kseg // 32, 32) * unit
        out.append((b * np.exp2(exp[:, col // 32:(col + kseg) // 32].astype(np.float64))[..., None]).reshape(-1, kseg))
        col += kseg
    return out


def pack(v, kind, wmode="w"):
    """(ON, OS, OO, SFN, SFS, SFO) as o.reorder_quantize returns them, written directly: element codes of base * 2^-e0 where e0 is the
    exponent the quantizer gives a block whose amax is the pin, and scale byte 127 + e0 + the block's own exponent"""
    base, exp, unit, pinv = (v.xbase, v.xexp, 1.0, X_PIN) if kind == "x" else (v.wbase, v.wexp, 0.5, W_PIN)
    fmts = X_FMTS if kind == "x" else w_formats(wmode)
    rows = base.shape[0]
    outs, sfs, col = [], [], 0
    for kseg, fmt in zip(v.split, fmts):
        e0 = int(o.scale_exponent(np.array([pinv], np.float32), fmt)[0])
        lut = o.encode(np.arange(-3, 7, dtype=np.float32) * np.float32(unit * 2.0 ** -e0), fmt)     # the oracle's encoder on the alphabet
        codes = lut[base[:, col:col + kseg] + np.int8(3)]
        outs.append(np.ascontiguousarray(_PACK[fmt](codes)).reshape(rows, o.packed_width(fmt, kseg)))
        sf = np.zeros((o.sf_size_x(rows, kseg) if kind == "x" else o.sf_size_w(rows, kseg),), np.uint8)
        if kseg and rows:
            r = np.arange(rows)[:, None]
            j = np.arange(kseg // 32)[None, :]
            sf[o.sf_offset(r, j, kseg)] = (127 + e0 + exp[:, col // 32:(col + kseg) // 32].astype(np.int32)).astype(np.uint8)
        sfs.append(sf)
        col += kseg
    return (*outs, *sfs)


def assert_lossless(q, v, kind, wmode="w"):
    """the packed operand decodes to the intended values, every element; returns o.dequant_operand's segments"""
    if q[0].shape[0] == 0:
        return None
    deq = o.dequant_operand(q, kind, wmode)
    for i, (got, want) in enumerate(zip(deq, segments(v, kind))):
        assert (got is None) == (want is None), (kind, wmode, i)
        if want is not None:
            assert got.shape == want.shape and np.array_equal(got, want), f"{kind} {wmode} segment {i}: the packing is not lossless"
    return deq


def product(x, w, device=None):
    """x @ w.T in fp64: numpy, or torch on `device`.  Exact for these values in any summation order, on any backend."""
    if device is None:
        return x @ w.T
    import torch
    return (torch.from_numpy(x).to(device) @ torch.from_numpy(w).to(device).T).cpu().numpy()


def segment_products(v, device=None):
    """the exact fp64 product of every present segment, in order"""
    return [product(x, w, device) for x, w in zip(segments(v, "x"), segments(v, "w")) if x is not None]


def _bf16(x):
    return o.bf16_to_f32(o.f32_to_bf16(np.asarray(x, dtype=np.float32)))


class Want(dict):
    """the expected outputs by name; the "+bias" ones are derived from the plain ones when first asked for"""

    def __init__(self, bias, items):
        super().__init__(items)
        self.bias = np.asarray(bias, dtype=np.float32)

    def __missing__(self, key):
        base, tail = key.split("+")
        assert tail == "bias"
        self[key] = o.f32_to_bf16(o.bf16_to_f32(self[base]) + self.bias[None, :])          # bf16(bf16(y) + bias)
        return self[key]


def rounding_chain(parts, bias, M, N):
    """the project's outputs from the exact per-segment products.  "reference": bf16 after each present segment, the running value
    carried in fp32; "fused": one bf16 rounding; "+bias": bf16(bf16(y) + bias); "f32": the exact sum.  bf16 results as bit patterns."""
    total = np.zeros((M, N), np.float64)
    d = np.zeros((M, N), np.float32)
    for p in parts:
        total += p
        d = _bf16((p + d.astype(np.float64)).astype(np.float32))       # fp32 accumulator + running value: exact (exactness_units)
    f32 = total.astype(np.float32)
    assert np.array_equal(f32.astype(np.float64), total)
    return Want(bias, {"reference": o.f32_to_bf16(d), "fused": o.f32_to_bf16(f32), "f32": f32})


def exactness_units(v, parts=None):
    """the largest |running value| + sum_k |x| |w| over all outputs and segments, in units of the smallest product bit (0.5).  fp32
    sums are exact in any order while this stays below 2^24.  With `parts` (the exact products) it is computed per output from the
    data; without, from the operands alone by Cauchy-Schwarz: |running| <= sum_k |x||w| <= |x_m| |w_n| summed over the segments so far."""
    xs, ws = segments(v, "x"), segments(v, "w")
    if parts is None:
        nx = sum(np.sqrt((x * x).sum(axis=1)).max() * np.sqrt((w * w).sum(axis=1)).max() for x, w in zip(xs, ws) if x is not None and len(x) and len(w))
        return 2.0 * nx / 0.5
    worst, run = 0.0, np.zeros((v.M, v.N))
    for p, (x, w) in zip(parts, [(x, w) for x, w in zip(xs, ws) if x is not None]):
        s = np.abs(x) @ np.abs(w).T
        worst = max(worst, float((np.abs(run) + s).max()) if s.size else 0.0)
        run = run + p                                                  # an upper bound of the rounded running value up to one bf16 ulp
        worst = max(worst, float(np.abs(run).max()) * (1 + 2.0 ** -8) if s.size else 0.0)
    return worst / 0.5


Case = namedtuple("Case", "values qx qw bias want")


def exact_case(M, N, split, wmode, seed, ranges=None, device=None, values=None, want=None):
    """One case: `qx`, `qw` the six packed activation / weight tensors (uint8 numpy, as o.reorder_quantize returns them), `bias` bf16
    bits [N], `want` the expected outputs (rounding_chain) and `values` the intended operands.  `values=` / `want=` reuse those of the
    other weight mode (the same when both modes share their exponent ranges); `device` runs the fp64 product with torch there."""
    ranges = tuple(ranges) if ranges is not None else RANGES[wmode]
    if values is None or values.ranges != ranges:
        values, want = exact_values(M, N, split, seed, ranges), None
    assert (values.M, values.N, values.split, values.seed) == (M, N, tuple(split), seed)
    qx, qw = pack(values, "x"), pack(values, "w", wmode)
    if want is None:
        want = rounding_chain(segment_products(values, device), values.bias, M, N)
    return Case(values, qx, qw, o.f32_to_bf16(values.bias), want)
