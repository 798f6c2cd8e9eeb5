"""Inputs of the sampler's exact-answer tests, shared by tests/test_sample_cpu.py (which proves their preconditions in fp64) and
tests/test_sample_gpu.py (which runs them).  Nothing here looks at what a kernel returned.

Filter cases: three classes -- 3 tokens at v1, 5 at v2, 1 000 at v3 < v2 < v1, the third at the HIGHEST indices -- over a background of
-inf or of the bf16 nearest v3 - 1000, drawn with u = 1 - 2^-24: the answer is the last token of the last class kept, and a kernel that ignores a filter
lands in the third class."""
import functools

import numpy as np

import sample_oracle as so

CHUNK = 8192
U_LAST = np.float32(1.0 - 2.0 ** -24)
MARGIN = 1e-3

# (name, (v1, v2, v3), T, vocab, background): every value a bf16
TRIPLES = [
    ("low byte", (8.0, 7.0, 6.0), 1.0, 1300, "-inf"),                  # keys 0xC080, 0xC060, 0xC040: one level-1 bin
    ("low byte, T = 0.5", (8.0, 7.0, 6.0), 0.5, 1300, "-inf"),
    ("low byte, T = 2", (8.0, 7.0, 6.0), 2.0, 1300, "lower"),
    ("three parts", (8.0, 7.0, 6.0), 1.0, 2 * CHUNK + 5, "lower"),
    ("high bytes", (8.0, 3.0, 0.5), 1.0, 1300, "-inf"),                # keys 0xC080, 0xBFC0, 0xBE80: three level-1 bins
    ("negative", (-6.0, -7.0, -8.0), 1.0, 1300, "lower"),              # keys 0x3EC0, 0x3EA0, 0x3E80
    ("negative high bytes", (-0.5, -3.0, -8.0), 2.0, 1300, "-inf"),
    ("both zeros", (0.0, -1.0, -2.0), 1.0, 1300, "-inf"),              # the first class mixes +0 and -0
]


def triple_row(values, vocab, background):
    """(bits [vocab], the last index of each class)"""
    v1, v2, v3 = values
    lower = so.values(so.bf16_bits(np.float32(v3 - 1000.0)))              # 1000 lower, to the nearest bf16: weight 0 at every T here
    x = np.full(vocab, -np.inf if background == "-inf" else lower, dtype=np.float32)
    third = np.arange(vocab - 1000, vocab)
    span = vocab - 1000
    first = np.array([7, span // 3, span - 50])
    second = np.array([3, 50, span // 2, span - 100, span - 10])
    x[third], x[second], x[first] = v3, v2, v1
    bits = so.bf16_bits(np.where(np.isfinite(x), x, 0.0))
    bits[~np.isfinite(x)] = 0xFF80
    if v1 == 0.0:
        bits[first[1]] = 0x8000                              # -0 between two +0
    assert np.array_equal(so.values(bits)[np.isfinite(x)], x[np.isfinite(x)].astype(np.float64)), "the values must be bf16"
    return bits, [int(first[-1]), int(second[-1]), int(third[-1])]


@functools.lru_cache(maxsize=None)
def filter_case(which):
    """the rows of one triple: (bits [vocab], T, [(label, k, p, q, classes kept)])"""
    name, values, T, vocab, background = TRIPLES[which]
    bits, last = triple_row(values, vocab, background)
    w = [float(np.exp((v - values[0]) / T)) for v in values]
    M = [3.0, 3.0 + 5.0 * w[1], 3.0 + 5.0 * w[1] + 1000.0 * w[2]]
    f32 = lambda x: float(np.float32(x))
    p_for = [f32(0.5 * M[0] / M[2]), f32(0.5 * (M[0] + M[1]) / M[2]), f32(0.5 * (M[1] + M[2]) / M[2])]
    q_for = [f32(np.sqrt(w[1])), f32(np.sqrt(w[1] * w[2])), f32(0.5 * w[2])]
    off = dict(k=0, p=1.0, q=0.0)
    rows = [("no filter", off["k"], off["p"], off["q"], 3)]
    rows += [(f"k = {k}", k, off["p"], off["q"], c) for k, c in ((3, 1), (4, 2), (8, 2), (9, 3), (1, 1), (1008, 3), (vocab, 3), (-5, 3))]
    rows += [(f"p for class {c + 1}", off["k"], p_for[c], off["q"], c + 1) for c in range(3)]
    rows += [("p = 0", off["k"], 0.0, off["q"], 1), ("p < 0", off["k"], -1.0, off["q"], 1), ("p NaN", off["k"], float("nan"), off["q"], 3),
             ("p = 1", off["k"], 1.0, off["q"], 3)]
    rows += [(f"q for class {c + 1}", off["k"], off["p"], q_for[c], c + 1) for c in range(3)]
    rows += [("q = 1", off["k"], off["p"], 1.0, 1), ("q > 1", off["k"], off["p"], 1.5, 3), ("q NaN", off["k"], off["p"], float("nan"), 3)]
    rows += [("all three, k binds", 4, f32(0.995), q_for[2], 2), ("all three, p binds", 9, p_for[0], q_for[2], 1),
             ("all three, q binds", 9, p_for[2], q_for[1], 2),
             # top-p counts from Z_k: with k = 8 the mass is M[1], and half of it lies inside the first class
             ("p of Z_k", 8, f32(0.5 * M[0] / M[1]), off["q"], 1), ("p of Z_k, class 2", 8, f32(0.5 * (M[0] + M[1]) / M[1]), off["q"], 2)]
    return bits, T, rows, last


def chosen_columns(vocab):
    """every edge of a row: the first and last 300 columns, +-9 around every multiple of CHUNK, +-1 around every multiple of 2 048"""
    cols = set(range(min(300, vocab))) | set(range(max(0, vocab - 300), vocab))
    for m in range(0, vocab + 10, CHUNK):
        cols |= set(range(m - 9, m + 10))
    for m in range(0, vocab + 2, 2048):
        cols |= {m - 1, m, m + 1}
    return sorted(c for c in cols if 0 <= c < vocab)
