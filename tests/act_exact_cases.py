"""Activation inputs whose quantized answer is known exactly, and the error bound of the device's silu_mul, for
tests/test_activate_exact_cpu.py, tests/test_activate_exact_gpu.py and tests/test_hw_gpu.py ("Exact-answer activation cases").

THE LOSSLESS GATE FAMILY.  silu_mul (csrc/mx_direct_convert.h) is x * rcp(1 + exp2(-x log2 e)) * b in fp32.  For a bf16 gate x >= 20,
exp2(-x log2 e) < 2^-28, so 1 + ex == 1.0 in fp32 whatever the last bits of the hardware exp2 are, rcp(1.0) == 1.0, and v = x * b:
the product of two 8-bit significands, exact in fp32 with up to 16 significand bits.  numpy's `o.silu_mul` returns the same bits
(test_activate_exact_cpu.py).  tests/test_hw_gpu.py::test_silu_mul_against_fp64 asserts the device half for every bf16 x >= 20.  Every
quantize32 site therefore has ONE right answer on these inputs -- `o.activate_quantize` byte for byte -- and the inputs can be placed on
the edges of the quantizer's arithmetic with twice the significand bits any bf16-valued exact test reaches:

  * every midpoint between adjacent codes at the block's scale (a tie: RNE decides), and the nearest 16-bit products on either side of
    it (closer than half a bf16 ulp: a quantizer that rounds through bf16, or compares truncated bits, decides them wrong);
  * amax == FMAX * 2^k (exponent k) and the nearest product above it (exponent k + 1: `mant > FMAX_MANT` on bits below bf16), the
    nearest product below it (rounds up onto the largest code);
  * amax on either side of the fp32 constant 1e-6f: at or below it the scale byte is 127 and every code is zero;
  * an all-zero block (+0 and -0: byte 127, the sign kept on the zero codes);
  * block scales 2^-20 .. 2^20 around the format's own exponent.
A value beyond FMAX * scale cannot reach the converters through quantize32 -- the exponent rule is exact, so amax / scale <= FMAX -- the
nearest edge is the value that rounds UP onto the largest code; what the converters do past FMAX with a free scale (the fp8 one does not
saturate by itself) is pinned by tests/test_hw_gpu.py::test_f32_converters_past_fmax.

All data is a pure function of (row, column, seed).

THE ERROR BOUND of silu_mul against the fp64 value x / (1 + e^-x) * b, for every other input (`silu_mul_bound`).  With t = -x log2 e,
ex = e^-x, and u = 2^-24 the unit roundoff of fp32:
  t_dev  = fl(x * fl32(log2 e))            = t (1 + d1)(1 + d2),  |d1|, |d2| <= u        -> 2^t_dev = ex * 2^(t (d1 + d2)),
                                             a relative error of |t| ln2 * 2^-23 to first order
  ex_dev = v_exp_f32(t_dev)                relative error u_exp on top
  s      = fl(1 + ex_dev)                  relative error ex / (1 + ex) * (|t| ln2 2^-23 + u_exp) + u
  r      = v_rcp_f32(s)                    relative error u_rcp on top
  v      = fl(fl(x * r) * b)               two more roundings of u
  total  <= ex / (1 + ex) * (|t| ln2 2^-23 + u_exp) + u_rcp + 3 * 2^-24,   times (1 + 2^-10) for the second-order terms.
u_exp = u_rcp = 2^-23: the instruction set reference ("AMD Instinct MI300 / CDNA3 Instruction Set Architecture", VOP1, V_EXP_F32 and
V_RCP_F32: "1ULP accuracy, denormals are flushed"; the CDNA4 guide repeats the entries), one ulp being at most 2^-23 of the value.
An fp32 multiply whose result is denormal rounds to 2^-149 instead: (|b| + 1) * 2^-150 absolute on top (the first product's error is
scaled by b).  FLUSH RANGES: v_exp_f32 overflows from t >= 128, and v_rcp_f32 returns 0 for a result below 2^-126, that is from
1 + 2^t > 2^126 on; from t >= 125.5 (one half: the errors of t_dev above are far smaller) the device may return anything between the
value and zero of its sign: the bound there is |v| itself plus the relative bound -- |v| <= 89 |b| 2^-125.5 in that range."""
import numpy as np

from oracle import mx_oracle as o

FMTS = ("fp4", "fp6", "fp8")
U_EXP = U_RCP = 2.0 ** -23
LOG2E = 1.4426950408889634
GATE_MIN = 20.0
F32_1EM6 = np.float32(1e-6)
_MASK = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------------------
# the bound
# ------------------------------------------------------------------------------------------------------------
def silu_mul_fp64(a_bits, b_bits):
    """x / (1 + e^-x) * b in fp64 (signed zeros kept; e^-x may overflow to inf: the quotient is then -0)"""
    x = o.bf16_to_f32(a_bits).astype(np.float64)
    b = o.bf16_to_f32(b_bits).astype(np.float64)
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(-x)) * b


def silu_mul_bound(a_bits, b_bits):
    """(relative bound d, absolute bound) per element: |device - v| <= d |v| + absolute, v = silu_mul_fp64 (module docstring)"""
    x = o.bf16_to_f32(a_bits).astype(np.float64)
    b = o.bf16_to_f32(b_bits).astype(np.float64)
    t = -x * LOG2E
    with np.errstate(over="ignore", invalid="ignore"):
        ex = np.exp(-x)
        w = np.where(np.isinf(ex), 1.0, ex / (1.0 + ex))
    d = (w * (np.abs(t) * np.log(2.0) * 2.0 ** -23 + U_EXP) + U_RCP + 3 * 2.0 ** -24) * (1 + 2.0 ** -10)
    absolute = (np.abs(b) + 1.0) * 2.0 ** -150
    flush = t >= 125.5
    v = np.abs(silu_mul_fp64(a_bits, b_bits))
    absolute = np.where(flush, v + absolute, absolute)
    return d, absolute


def rule_exponent(amax64, fmt):
    """the exponent rule on a real amax > 1e-6 (fp64): the smallest e with FMAX * 2^e >= amax, clamped"""
    fmax = o.FORMATS[fmt]["fmax"]
    with np.errstate(divide="ignore"):
        e = np.ceil(np.log2(amax64 / fmax))
    # log2 of an exact FMAX * 2^k is exact in fp64 for these magnitudes; guard the comparison anyway
    e = np.where(fmax * np.exp2(e - 1) >= amax64, e - 1, e)
    e = np.where(fmax * np.exp2(e) < amax64, e + 1, e)
    return np.clip(e, -127, 127).astype(np.int64)


def admissible(v64, d, absolute, sf_bytes, fmt):
    """For fp64 values v [rows, kseg] with bounds d / absolute and the scale bytes the DEVICE wrote ([rows, kseg / 32]):
    (byte_ok [rows, kseg / 32], code_lo, code_hi [rows, kseg]).
    The device's values are fp32 numbers v' with |v' - v| <= err = d |v| + absolute, so its amax lies in [max(|v| - err), max(|v| + err)]
    over the block; the exponent rule is monotone, so byte_ok asks for a byte between the rule's exponents of the two ends (127 -- scale
    1.0 -- when an admissible amax is <= 1e-6f).  code_lo / code_hi: the RNE codes, at the DEVICE's scale, of the smallest and the largest
    fp32 inside [v - err, v + err]; RNE is monotone, so the device's code lies between them on the value axis (`code_pos`), and the
    interval is so much narrower than a code step that they are equal or adjacent (test_activate_exact_cpu.py asserts that)."""
    rows, kseg = v64.shape
    err = d * np.abs(v64) + absolute
    g = np.abs(v64).reshape(rows, kseg // 32, 32)
    ge = err.reshape(rows, kseg // 32, 32)
    lo, hi = np.maximum(g - ge, 0.0).max(-1), (g + ge).max(-1)
    e_dev = sf_bytes.astype(np.int64) - 127
    thr = float(F32_1EM6)
    above = np.nextafter(thr, 1.0)
    ok_rule = (hi > thr) & (e_dev >= rule_exponent(np.maximum(lo, above), fmt)) & (e_dev <= rule_exponent(np.maximum(hi, above), fmt))
    ok_empty = (lo <= thr) & (e_dev == 0)
    scale = np.exp2(-np.maximum(e_dev, -126).astype(np.float64))[..., None]
    fmax = o.FORMATS[fmt]["fmax"]
    ends = []
    for end, toward in ((v64 - err, np.inf), (v64 + err, -np.inf)):
        # an end that crosses zero stops at the zero of v's sign: x * r * b never changes sign
        end = np.where(np.signbit(end) != np.signbit(v64), np.copysign(0.0, v64), end)
        q = np.clip(end.reshape(rows, kseg // 32, 32) * scale, -fmax, fmax)
        f = q.astype(np.float32)                                  # the nearest fp32 ...
        outside = (f.astype(np.float64) < q) if toward > 0 else (f.astype(np.float64) > q)
        f = np.where(outside, np.nextafter(f, np.float32(toward)), f)   # ... moved inside the interval where it fell outside
        ends.append(o.encode(f.reshape(rows, kseg), fmt))
    return ok_rule | ok_empty, ends[0], ends[1]


def code_pos(codes, fmt):
    """sign-magnitude codes -> position on the value axis (-0 one step below +0)"""
    sbit = 1 << (o.FORMATS[fmt]["bits"] - 1)
    c = np.asarray(codes).astype(np.int64)
    return np.where(c & sbit, -(c & (sbit - 1)) - 1, c & (sbit - 1))


# ------------------------------------------------------------------------------------------------------------
# the lossless family
# ------------------------------------------------------------------------------------------------------------
def _hash(a, b, salt):
    """splitmix64 finaliser over (a, b, salt), vectorised; a and b broadcast (as tests/gemm_exact_cases.py)"""
    s = np.uint64((salt * 0xD6E8FEB86659FD93 + 0x2545F4914F6CDD1D) & _MASK)
    h = (np.asarray(a, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ (np.asarray(b, dtype=np.uint64) * np.uint64(0xC2B2AE3D27D4EB4F)) ^ s
    h = (h ^ (h >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    h = (h ^ (h >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return h ^ (h >> np.uint64(31))


def _product_table():
    """every value g * u * 2^s (g, u = 128 .. 255 the significands of two bf16, s = -1, 0, 1), sorted, with one (g, u, s) each"""
    g, u = np.meshgrid(np.arange(128, 256), np.arange(128, 256), indexing="ij")
    vals, gs, us, ss = [], [], [], []
    for s in (-1, 0, 1):
        vals.append((g * u).astype(np.float64).ravel() * 2.0 ** s)
        gs.append(g.ravel()); us.append(u.ravel()); ss.append(np.full(g.size, s))
    vals, gs, us, ss = (np.concatenate(x) for x in (vals, gs, us, ss))
    vals, first = np.unique(vals, return_index=True)
    return vals, gs[first], us[first], ss[first]


_TABLE = _product_table()


def _spec(value, side=0):
    """(g, u, x) with g * u * 2^x the product equal to `value` (side 0; it must exist), the nearest below (-1) or above (+1)"""
    x = int(np.floor(np.log2(value))) - 15
    m = value / 2.0 ** x                                     # in [2^15, 2^16)
    vals, gs, us, ss = _TABLE
    i = int(np.searchsorted(vals, m))
    if side == 0:
        assert vals[i] == m, f"{value} is no product of two bf16 significands"
    elif side < 0:
        i -= 1
    elif vals[i] == m:
        i += 1
    return int(gs[i]), int(us[i]), int(ss[i]) + x


def _bits(spec):
    """(gate bits, up bits) of a spec: gate = g / 4 in [32, 64), up = u * 2^(x + 2)"""
    if spec is None:
        return (132 << 7), 0                                 # gate 32, up +0
    g, u, x = spec
    ef = 136 + x
    assert 1 <= ef - 24 and ef + 24 <= 254
    return (132 << 7) | (g - 128), (ef << 7) | (u - 128)


def spec_value(spec):
    return 0.0 if spec is None else spec[0] * spec[1] * 2.0 ** spec[2]


def midpoints(fmt):
    """the midpoints between adjacent non-negative codes, ascending (the first is half the smallest subnormal)"""
    vals = o.decode(np.arange(o.FORMATS[fmt]["maxcode"] + 1, dtype=np.uint8), fmt).astype(np.float64)
    return (vals[:-1] + vals[1:]) / 2


def unit_blocks(fmt):
    """the edge blocks of one format at block exponent 0 (amax = FMAX): (gate bits [nb, 32], up bits [nb, 32], shiftable [nb]).
    Element 0 of a block is its amax; `family` rotates the positions."""
    fmax = o.FORMATS[fmt]["fmax"]
    triples = [[_spec(m, -1), _spec(m, 0), _spec(m, +1)] for m in midpoints(fmt)]
    flat = [s for t in triples for s in t]
    # (the ties of the lower half only: doubled, the others would pass the block's amax)
    up1 = lambda s: (s[0], s[1], s[2] + 1) if s is not None and 2 * spec_value(s) < fmax else None
    pad = lambda blk: blk + [None] * (32 - len(blk))
    blocks, shiftable = [], []
    for at in range(0, len(flat), 30):
        fill = flat[at:at + 30]
        blocks.append(pad([_spec(fmax, 0)] + fill))                      # amax = FMAX exactly: exponent 0, ties at scale 1
        blocks.append(pad([_spec(fmax, +1)] + [up1(s) for s in fill]))   # amax one product above FMAX: exponent 1, ties at scale 2
        shiftable += [True, True]
    blocks.append(pad([_spec(fmax, -1)] + flat[-30:]))                   # amax one product below FMAX: rounds up onto the largest code
    shiftable.append(True)
    # amax on either side of the fp32 constant 1e-6f; smaller products and zeros around it
    rng = np.random.default_rng(106)
    thr = float(F32_1EM6)
    for side in (-1, +1):
        pin = _spec(thr, side)
        small = [(int(rng.integers(128, 256)), int(rng.integers(128, 256)), pin[2] - int(rng.integers(2, 6))) for _ in range(24)]
        blocks.append(pad([pin] + small))
        shiftable.append(False)
    blocks.append([None] * 32)                                       # the all-zero block
    shiftable.append(False)
    x0 = int(np.floor(np.log2(fmax))) - 15
    for _ in range(4):                                               # full 16-bit products over a few binades
        blocks.append([(int(rng.integers(128, 256)), int(rng.integers(128, 256)), x0 - int(rng.integers(0, 7))) for _ in range(32)])
        shiftable.append(True)
    gb = np.array([[_bits(s)[0] for s in blk] for blk in blocks], dtype=np.uint16)
    ub = np.array([[_bits(s)[1] for s in blk] for blk in blocks], dtype=np.uint16)
    return gb, ub, np.array(shiftable)


_UNITS = {}


def family(rows, split, seed=0, row0=0):
    """(gate bits, up bits) uint16 [rows, K] of the lossless family: segment s walks the edge blocks of its format in order, block
    (r, j) shifted by 2^-20 .. 2^20 (a hash; not the 1e-6 and zero blocks), its 32 positions rotated and its signs drawn by further
    hashes of (row0 + r, j)"""
    K = sum(split)
    gate = np.zeros((rows, K), np.uint16)
    up = np.zeros((rows, K), np.uint16)
    r = (row0 + np.arange(rows, dtype=np.int64))[:, None]
    col = 0
    for si, (kseg, fmt) in enumerate(zip(split, FMTS)):
        if not kseg:
            continue
        if fmt not in _UNITS:
            _UNITS[fmt] = unit_blocks(fmt)
        gb, ub, shiftable = _UNITS[fmt]
        nb, nseg = len(gb), kseg // 32
        j = np.arange(nseg, dtype=np.int64)[None, :]
        pick = (r * nseg + j + seed) % nb
        h = _hash(r, j + 4096 * si, 8 * seed + 1)
        shift = np.where(shiftable[pick], (h % np.uint64(41)).astype(np.int64) - 20, 0)
        rot = ((h >> np.uint64(8)) % np.uint64(32)).astype(np.int64)
        sign = (((h >> np.uint64(16)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
        src = (np.arange(32)[None, None, :] - rot[..., None]) % 32          # position p holds element (p - rot) % 32
        g = np.take_along_axis(gb[pick], src, -1)
        u = np.take_along_axis(ub[pick], src, -1).astype(np.int64)
        u = np.where(u != 0, u + (shift[..., None] << 7), 0) | (sign.astype(np.int64) << 15)
        gate[:, col:col + kseg] = g.reshape(rows, kseg)
        up[:, col:col + kseg] = u.astype(np.uint16).reshape(rows, kseg)
        col += kseg
    return gate, up


def interleave(gate, up):
    """[rows, 2 K]: 128 gate | 128 up columns alternating -- the matrix mm_down_activate_decode and the M <= 64 scratch take"""
    rows, K = gate.shape
    return np.stack([gate.reshape(rows, K // 128, 128), up.reshape(rows, K // 128, 128)], axis=2).reshape(rows, 2 * K)


# (rows, K, split) of tests/test_activate_exact_gpu.py part a; LARGE is the smallest row count of a 8448-wide matrix whose groups the
# grid-stride loop of direct_quantize_kernel (at most 4096 workgroups of 256 groups) needs a second trip for
CASES = [(37, 128, (0, 128, 0)), (5, 384, (128, 128, 128)), (130, 1024, (512, 128, 384))]
TRIP_GROUPS = 4096 * 256
LARGE = (4096, 8448, (4096, 2048, 2304))
# the Gaussian cases of tests/test_direct_quantize_gpu.py::test_activate_quantize_close_to_oracle
GAUSSIAN = [(7, 384, (128, 128, 128)), (130, 4096, (2048, 1024, 1024)), (48, 14336, (12288, 1024, 1024))]
AMBIGUOUS_CAP = 1e-3


def gaussian_case(rows, k):
    """the inputs of test_activate_quantize_close_to_oracle, bit for bit (same generator, same order of draws)"""
    rng = np.random.default_rng(k + rows)
    ab = o.f32_to_bf16((rng.standard_normal((rows, k)) * 2).astype(np.float32))
    x = rng.standard_normal((rows, k)).astype(np.float32)
    cols = rng.choice(k, size=max(1, k // 100), replace=False)
    x[:, cols] *= 20.0
    return ab, o.f32_to_bf16(x)


def all_gate_case(split=(128, 128, 128)):
    """gate runs over every finite bf16 (one per row of each column block), up N(0, 1) with outliers"""
    allb = np.arange(65536, dtype=np.uint16)
    fin = allb[np.isfinite(o.bf16_to_f32(allb))]
    k = sum(split)
    rows = -(-len(fin) // k)
    ab = np.resize(fin, (k, rows)).T.copy()           # a gate COLUMN runs through consecutive bf16
    rng = np.random.default_rng(65536)
    x = rng.standard_normal((rows, k)).astype(np.float32)
    x[:, ::97] *= 20.0
    ub = o.f32_to_bf16(x)
    # inf is out of scope: where |gate| >= 2^100 the up value is taken 2^-30 smaller, so that no product overflows
    big = ((ab >> 7) & 0xFF) >= 227
    return ab, np.where(big & (((ub >> 7) & 0xFF) > 40), ub - np.uint16(30 << 7), ub).astype(np.uint16)


# ------------------------------------------------------------------------------------------------------------
# one-hot gate / up weights: the fused launches copy chosen activation values into gate and up
# ------------------------------------------------------------------------------------------------------------
def onehot_case(M, H, I, seed=0):
    """(x [M, H], w_gate [I, H], w_up [I, H], gate [M, I], up [M, I]) as bf16 bits.  The rows of x are written in the alphabet of
    tests/gemm_exact_cases.py, lossless under reorder_quantize_x with the identity index in every format: an even 32-block holds
    {1, 2, 3} * 32 and one 6 * 32 (gate material, all >= 32), an odd block integers -3 .. 3 and one 6, times 2^s with s a hash of
    (row, block) in -34 .. 8, so that output blocks fall on either side of 1e-6.  Row i of w_gate / w_up is 1.0 in one column and 0
    elsewhere (lossless in fp4: 4 * 2^-2), so gate[m, i] = x[m, kg(i)] and up[m, i] = x[m, ku(i)] exactly, through any summation order
    and either rounding of the GEMM; the 32 features of an output block draw from one even and one odd block of x."""
    nb = H // 32
    r = np.arange(M, dtype=np.int64)[:, None]
    c = np.arange(H, dtype=np.int64)[None, :]
    blk = np.arange(nb, dtype=np.int64)[None, :]
    h = _hash(r, c, 16 * seed + 3)
    even = ((c // 32) % 2 == 0)
    base = np.where(even, (h % np.uint64(3)).astype(np.int64) + 1, (h % np.uint64(7)).astype(np.int64) - 3)
    pin = (_hash(r, blk, 16 * seed + 4) % np.uint64(32)).astype(np.int64)
    np.put_along_axis(base.reshape(M, nb, 32), pin[..., None], 6, axis=2)
    s = np.where(blk % 2 == 0, 5, (_hash(r, blk, 16 * seed + 5) % np.uint64(43)).astype(np.int64) - 34)
    xv = (base.reshape(M, nb, 32) * np.exp2(s.astype(np.float64))[..., None]).reshape(M, H)
    x = o.f32_to_bf16(xv.astype(np.float32))
    assert np.array_equal(o.bf16_to_f32(x).astype(np.float64), xv)
    i = np.arange(I, dtype=np.int64)
    ob = i // 32
    kg = 32 * (2 * (_hash(ob, 0, 16 * seed + 6) % np.uint64(nb // 2)).astype(np.int64)) + (_hash(i, 1, 16 * seed + 7) % np.uint64(32)).astype(np.int64)
    ku = 32 * (2 * (_hash(ob, 2, 16 * seed + 8) % np.uint64(nb // 2)).astype(np.int64) + 1) + (_hash(i, 3, 16 * seed + 9) % np.uint64(32)).astype(np.int64)
    wg = np.zeros((I, H), np.uint16)
    wu = np.zeros((I, H), np.uint16)
    wg[i, kg] = 0x3F80
    wu[i, ku] = 0x3F80
    return x, wg, wu, x[:, kg].copy(), x[:, ku].copy()


# (site, M, H, I, in_split, down_split) of tests/test_activate_exact_gpu.py part d; the wide layer has 2 I / 64 = 256 workgroups, one
# per CU of an MI355X, which is where mm_gate_up_activate takes the one-launch streaming form
ONEHOT = [("scratch", 40, 384, 512, (128, 128, 128), (256, 128, 128)),
          ("tile", 130, 384, 512, (128, 128, 128), (256, 128, 128)),
          ("stream1", 3, 1024, 8192, (512, 128, 384), (4096, 2048, 2048)),
          ("stream2", 27, 1024, 8192, (512, 128, 384), (4096, 2048, 2048))]
