"""The RMSNorm sum of squares taken in the WRONG order, and the rows that notice (tests/golden/rms_sentinels.json).

oracle/mx_oracle.py: rmsnorm_rvar fixes one order of fp32 additions: group thread t of T = K/32 adds the squares of elements
i*K/4 + 8t + j one after the other, and the T partial sums meet in the halving tree over the next power of two.  Every function of
SUM_ORDERS below is a plain numpy restatement of an order a kernel could have instead -- each one is what a natural way of writing
the reduction computes -- and returns the sum of squares of every row; rvars() turns them into rvar.  On Gaussian rows these move
rvar by one ulp in 1 to 50 % of the rows, and one ulp of rvar changes an output byte of the quantizer in one row of 30 000 (K = 128) to one of 80 (K = 16512): a
test on a few hundred random rows passes with any of them.  A SENTINEL is a row whose oracle output bytes differ between the
oracle's rvar and a wrong one; the fixture holds at least two per (K, integer_round, wrong order), found by
tests/golden/make_rms_sentinels.py, and tests/test_rms_sentinels_cpu.py re-derives each of them.

Rows, norm weights and reorder indices are functions of integer seeds through the LCG of tests/golden/lcg.py, so the fixture holds no
bits and nothing depends on numpy's random stream.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import lcg  # noqa: E402
from oracle import mx_oracle as o  # noqa: E402

EPS = 1e-5
FIXTURE = os.path.join(HERE, "golden", "rms_sentinels.json")

# K -> split: one K per code path and per thread count of the quantizer's kernels (T = K/32 group threads)
SPLITS = {128: (0, 0, 128),                  # T = 4: one wave, a tree that is mostly padding
          2176: (1024, 128, 1024),           # T = 68: two waves, P = 128
          4096: (2048, 1024, 1024),          # T = 128
          4224: (2048, 128, 2048),           # T = 132: three waves, P = 256
          8192: (4096, 2048, 2048),          # T = 256: the largest K of the 32-bit product row
          8320: (4096, 128, 4096),           # T = 260: the 16-bit row, 320 threads
          16384: (8192, 4096, 4096),         # T = 512
          16512: (8192, 128, 8192),          # T = 516: two groups per thread, 320 threads
          20480: (8192, 4096, 8192),         # T = 640: 320 threads
          24576: (8192, 8192, 8192),         # T = 768: 384 threads
          28672: (12288, 4096, 12288),       # T = 896: 448 threads
          32768: (16384, 8192, 8192)}        # T = 1024: 512 threads


# ---- seeded inputs --------------------------------------------------------------------------------------------------------------
_A, _C, _M64 = 6364136223846793005, 1442695040888963407, (1 << 64) - 1
_BLOCK = 1 << 16
_table = None


def _lcg_table():
    """state after i + 1 steps from s is mul[i] * s + add[i] (as lcg.lcg_u32 builds it on every call; here once)"""
    global _table
    if _table is None:
        mul, add = np.empty(_BLOCK, np.uint64), np.empty(_BLOCK, np.uint64)
        m, a = 1, 0
        for i in range(_BLOCK):
            m, a = (m * _A) & _M64, (a * _A + _C) & _M64
            mul[i], add[i] = m, a
        _table = (mul, add)
    return _table


def lcg_words(seed: int, first: int, n: int) -> np.ndarray:
    """lcg.lcg_u32(seed, first + n)[first:], without generating the first `first` words: the LCG jumps ahead by squaring"""
    m, a, pm, pa, k = 1, 0, _A, _C, first                # s -> m s + a after `first` steps
    while k:
        if k & 1:
            m, a = (pm * m) & _M64, (pm * a + pa) & _M64
        pm, pa = (pm * pm) & _M64, (pm * pa + pa) & _M64
        k >>= 1
    s = np.uint64((m * seed + a) & _M64)
    mul, add = _lcg_table()
    out = np.empty(n, np.uint32)
    pos = 0
    with np.errstate(over="ignore"):
        while pos < n:
            st = mul * s + add
            take = min(_BLOCK, n - pos)
            out[pos:pos + take] = (st[:take] >> np.uint64(32)).astype(np.uint32)
            s = st[_BLOCK - 1]
            pos += take
    return out


def _bell(words: np.ndarray) -> np.ndarray:
    """uint32 words -> roughly N(0, 1) fp32: the sum of the four bytes, centred and scaled (std of four uniform bytes: 147.8)"""
    w = words.astype(np.int64)
    total = (w & 0xFF) + ((w >> 8) & 0xFF) + ((w >> 16) & 0xFF) + (w >> 24)
    return ((total - 510).astype(np.float32) / np.float32(147.8)).astype(np.float32)


def seeded_rows(k: int, first: int, n: int) -> np.ndarray:
    """rows first .. first + n - 1 of the row stream of K = k, bf16 bit patterns [n, k]: row i is words [i k, (i + 1) k) of LCG seed k"""
    return o.f32_to_bf16(_bell(lcg_words(k, first * k, n * k))).reshape(n, k)


def seeded_row(k: int, i: int) -> np.ndarray:
    return seeded_rows(k, i, 1)[0]


def norm_weight(k: int) -> np.ndarray:
    """the norm weight of every sentinel of K = k: bf16(1 + 0.2 N(0, 1)), LCG seed 1000003 + k"""
    return o.f32_to_bf16((np.float32(1.0) + np.float32(0.2) * _bell(lcg_words(1000003 + k, 0, k))).astype(np.float32))


def reorder_index(k: int) -> np.ndarray:
    """the reorder index of every sentinel of K = k: lcg.permutation, seed 2000003 + k"""
    return lcg.permutation(2000003 + k, k)


# ---- the pieces of the sum -----------------------------------------------------------------------------------------------------
def _f32(a):
    return np.asarray(a, np.float32)


def squares(x_bits):
    x = o.bf16_to_f32(np.atleast_2d(np.asarray(x_bits)))
    return (x * x).astype(np.float32)                     # exact


def thread_partials(sq, chunks=(0, 1, 2, 3)):
    """[rows, T]: group thread t adds the squares of its chunks, in the given order of chunks, eight elements each, one after the other"""
    rows, k = sq.shape
    t = k // 32
    part = np.zeros((rows, t), np.float32)
    for i in chunks:
        blk = sq[:, i * (k // 4):(i + 1) * (k // 4)].reshape(rows, t, 8)
        for j in range(8):
            part = _f32(part + blk[:, :, j])
    return part


def pow2_at_least(n):
    p = 1
    while p < n:
        p *= 2
    return p


def halving_tree(part, p=None):
    """s[t] += s[t + stride], stride = P/2 .. 1, over P >= T slots, zero padded: [rows]"""
    rows, t = part.shape
    p = pow2_at_least(t) if p is None else p
    s = np.zeros((rows, p), np.float32)
    s[:, :t] = part
    stride = p // 2
    while stride >= 1:
        s[:, :stride] = _f32(s[:, :stride] + s[:, stride:2 * stride])
        stride //= 2
    return s[:, 0].copy()


def finish(total, k, eps=EPS):
    mean = _f32(_f32(total) / np.float32(k))
    return _f32(np.float32(1.0) / np.sqrt(_f32(mean + np.float32(eps))))


def launch_threads(k):
    """threads of the quantizer's launch (launch_rmsnorm_quantize): one group per thread up to K = 16384, two beyond, whole waves"""
    t = k // 32
    gpt = 2 if t > 512 else 1
    return ((t + gpt - 1) // gpt + 63) // 64 * 64


# ---- the wrong orders: (squares [rows, K], the oracle's partial sums [rows, T]) -> sum of squares [rows] -----------------------------
def fp64_sum(sq, part):
    """the sum in double precision, rounded once"""
    return sq.astype(np.float64).sum(axis=1).astype(np.float32)


def chunks_reversed(sq, part):
    """a thread adds its four chunks last to first"""
    return halving_tree(thread_partials(sq, (3, 2, 1, 0)))


def contiguous_32(sq, part):
    """thread t adds the 32 contiguous elements 32t .. 32t + 31 instead of four chunks K/4 apart"""
    rows, k = sq.shape
    blk = sq.reshape(rows, k // 32, 32)
    mine = np.zeros((rows, k // 32), np.float32)
    for j in range(32):
        mine = _f32(mine + blk[:, :, j])
    return halving_tree(mine)


def partials_sequential(sq, part):
    """the T partial sums added one after the other instead of in the tree"""
    s = np.zeros(sq.shape[0], np.float32)
    for t in range(part.shape[1]):
        s = _f32(s + part[:, t])
    return s


def adjacent_tree(sq, part):
    """a tree over adjacent pairs, s[t] = s[2t] + s[2t + 1], instead of over halves"""
    rows, t = part.shape
    s = np.zeros((rows, pow2_at_least(t)), np.float32)
    s[:, :t] = part
    while s.shape[1] > 1:
        s = _f32(s[:, 0::2] + s[:, 1::2])
    return s[:, 0]


def dword_pairs(sq, part):
    """the two elements of a dword summed first, then added to the running sum"""
    rows, k = sq.shape
    t = k // 32
    mine = np.zeros((rows, t), np.float32)
    for i in range(4):
        blk = sq[:, i * (k // 4):(i + 1) * (k // 4)].reshape(rows, t, 8)
        for j in range(0, 8, 2):
            mine = _f32(mine + _f32(blk[:, :, j] + blk[:, :, j + 1]))
    return halving_tree(mine)


def dword_halves_swapped(sq, part):
    """the high half of every dword added before the low half: elements 1, 0, 3, 2, ... of a chunk"""
    rows, k = sq.shape
    t = k // 32
    mine = np.zeros((rows, t), np.float32)
    for i in range(4):
        blk = sq[:, i * (k // 4):(i + 1) * (k // 4)].reshape(rows, t, 8)
        for j in (1, 0, 3, 2, 5, 4, 7, 6):
            mine = _f32(mine + blk[:, :, j])
    return halving_tree(mine)


def fold_two_groups(sq, part):
    """K > 16384, two groups per thread: s[g] + s[g + NTH] in registers before the tree over the NTH sums (NTH: the launch's threads).
    With one group per thread there is nothing to fold: the oracle's order."""
    rows, t = part.shape
    nth = launch_threads(sq.shape[1])
    if t <= 512:
        return halving_tree(part)
    two = np.zeros((rows, 2 * nth), np.float32)
    two[:, :t] = part
    return halving_tree(_f32(two[:, :nth] + two[:, nth:]))


def pad_to_64(sq, part):
    """padded to whole waves instead of a power of two: lane l adds s[l], s[l + 64], s[l + 128], ... one after the other, then the
    tree over the 64 lanes"""
    rows, t = part.shape
    n = (t + 63) // 64
    s = np.zeros((rows, n * 64), np.float32)
    s[:, :t] = part
    lanes = s[:, :64].copy()
    for w in range(1, n):
        lanes = _f32(lanes + s[:, 64 * w:64 * w + 64])
    return halving_tree(lanes)


def lane_pair(sq, part):
    """the decode chain done wrong: chunks 0, 1 and chunks 2, 3 summed separately from zero by the two lanes of a pair, then added"""
    return halving_tree(_f32(thread_partials(sq, (0, 1)) + thread_partials(sq, (2, 3))))


def waves_first(sq, part):
    """each 64 consecutive partial sums reduced by the shuffle ladder of their wave, then the tree across the waves' results"""
    rows, t = part.shape
    n = (t + 63) // 64
    s = np.zeros((rows, n * 64), np.float32)
    s[:, :t] = part
    return halving_tree(np.stack([halving_tree(s[:, 64 * w:64 * w + 64]) for w in range(n)], axis=1))


SUM_ORDERS = {f.__name__: f for f in (fp64_sum, chunks_reversed, contiguous_32, partials_sequential, adjacent_tree, dword_pairs, dword_halves_swapped,
                                      fold_two_groups, pad_to_64, lane_pair, waves_first)}
# the two that need no order at all: nextafter(rvar, +inf) and nextafter(rvar, -inf)
ORDERS = tuple(SUM_ORDERS) + ("ulp_up", "ulp_down")


def oracle_order(sq, part):
    return halving_tree(part)


def rvars(x_bits, names=ORDERS, eps=EPS):
    """(the oracle's rvar [rows], {name: that order's rvar [rows]}) -- the squares and the oracle's partial sums are taken once"""
    sq = squares(x_bits)
    part = thread_partials(sq)
    k = sq.shape[1]
    right = finish(oracle_order(sq, part), k, eps)
    wrong = {}
    for name in names:
        if name == "ulp_up":
            wrong[name] = np.nextafter(right, np.float32(np.inf)).astype(np.float32)
        elif name == "ulp_down":
            wrong[name] = np.nextafter(right, np.float32(-np.inf)).astype(np.float32)
        else:
            wrong[name] = finish(SUM_ORDERS[name](sq, part), k, eps)
    return right, wrong


# ---- what a wrong rvar does to the output ----------------------------------------------------------------------------------------
def normalised_bits(x_bits, w_bits, idx, rvar):
    """bf16((x w) rvar) of the reordered row(s): what the quantizer sees -- the cheap screen for a row that notices another rvar"""
    xv = o.bf16_to_f32(np.atleast_2d(np.asarray(x_bits)))[:, idx]
    wv = o.bf16_to_f32(np.asarray(w_bits))[idx]
    return o.f32_to_bf16(_f32(_f32(xv * wv[None, :]) * _f32(rvar)[:, None]))


def codes_of(outs, split):
    """the six oracle outputs of `rows` rows -> ([rows, K] element codes in reordered order, [rows, K/32] scale bytes)"""
    rows = outs[0].shape[0]
    codes, scales = [], []
    for packed, sf, kseg, fmt in zip(outs[:3], outs[3:], split, ("fp4", "fp6", "fp8")):
        if kseg:
            codes.append(o._UNPACK[fmt](packed))
            scales.append(sf[o.sf_valid_offsets(rows, kseg)].reshape(rows, kseg // 32))
    return np.concatenate(codes, axis=1), np.concatenate(scales, axis=1)


def flip_column(x_bits, k, integer_round, rvar_wrong):
    """the first reordered column of ONE row whose code differs between the oracle's rvar and `rvar_wrong`, -1 if no output byte
    differs at all, -2 if only scale bytes do"""
    split, w, idx = SPLITS[k], norm_weight(k), reorder_index(k)
    x = np.asarray(x_bits).reshape(1, k)
    right = codes_of(o.rmsnorm_quantize(x, w, EPS, idx, *split, integer_round=integer_round), split)
    wrong = codes_of(o.rmsnorm_quantize(x, w, EPS, idx, *split, integer_round=integer_round, rvar=rvar_wrong), split)
    cols = np.flatnonzero(right[0][0] != wrong[0][0])
    if len(cols):
        return int(cols[0])
    return -1 if np.array_equal(right[1], wrong[1]) else -2


DECODE_KS = (128, 4096, 4224, 8192)      # the K at which the decode launches that carry the norm are tested (they take K <= 8192)


def one_hot_output_differs(x_bits, k, integer_round, rvar_wrong, column):
    """a weight row that is one-hot at reordered position `column`: does the oracle product of ONE row's codes with it differ between
    the oracle's rvar and `rvar_wrong`, in both weight modes?  (tests/test_rms_order_decode_gpu.py builds its weights so)"""
    split, w, idx = SPLITS[k], norm_weight(k), reorder_index(k)
    x = np.asarray(x_bits).reshape(1, k)
    hot = np.zeros((1, k), np.uint16)
    hot[0, int(idx[column])] = 0x3F80                    # 1.0
    good_q = o.rmsnorm_quantize(x, w, EPS, idx, *split, integer_round=integer_round)
    bad_q = o.rmsnorm_quantize(x, w, EPS, idx, *split, integer_round=integer_round, rvar=rvar_wrong)
    for wmode in ("w4", "w"):
        qw = o.reorder_quantize(hot, idx, *split, wmode)
        good = o.matmul(*[t for pair in zip(good_q, qw) for t in pair])
        wrong = o.matmul(*[t for pair in zip(bad_q, qw) for t in pair])
        if good.shape != (1, 1) or good[0, 0] == wrong[0, 0]:
            return False
    return True


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def sentinel_rows(fixture, k, integer_round):
    """the distinct row numbers of the sentinels of (K, integer_round), in the fixture's order"""
    seen = []
    for s in fixture["sentinels"]:
        if s["K"] == k and s["integer_round"] == integer_round and s["row"] not in seen:
            seen.append(s["row"])
    return seen
