"""The sparse MoE block (micromix_amd.moe.SparseMoEBlock) restated in numpy on bf16 bit patterns, the configurations its block tests run,
and a builder of inputs whose routing is prescribed.

configs   CONFIGS: five blocks with H != I, split1 != split2 and empty segments, both weight modes, both roundings, experts with and
          without biases; SCRIPTED: the rows per expert each of them is run with (streaming tiers <= 16 / 32 / 48 / 64, both sides of
          the 64 / 65 change of kernel, a group past one 128-row tile, empty experts, E = 16 and 64: several launches per grouped call)
builder   scripted_x: gate_weight[e] is the unit vector of column e, and the first E columns of x hold the routing values -- token t has
          4, 2, 1, 0.5, ... on its chosen experts in k-slot order and -4 elsewhere.  Every product of the gate linear is a power of two
          or zero, so the logits are exact in whatever order a bf16 linear sums, and the routing is the prescribed one.
oracle    oracle_block: moe_oracle.route / plan / combine around o.reorder_quantize(.., "x") and o.matmul per expert, the bias added
          the reference's way (y = bf16(y + bias), qLinearLayer.py:70-71), h = bf16(bf16(silu(a)) * b) with silu in fp64 and two
          roundings.  unquantized_block: the same routing through fp64 products of the bf16 weights, nothing rounded.
"""
from __future__ import annotations

import numpy as np

import moe_oracle as mo
from oracle import mx_oracle as o

# split1 is over H (w1 / w3 read it), split2 over I (w2 reads it); bias: which experts / layers carry one
CONFIGS = {
    "A": dict(E=8, k=2, H=256, I=512, split1=(128, 0, 128), split2=(256, 128, 128), wmode="w4", rounding="reference", bias="none"),
    "B": dict(E=16, k=4, H=384, I=256, split1=(128, 128, 128), split2=(0, 128, 128), wmode="w", rounding="fused", bias="odd experts"),
    "C": dict(E=64, k=8, H=256, I=384, split1=(128, 128, 0), split2=(128, 128, 128), wmode="w4", rounding="reference", bias="w2"),
    "D": dict(E=3, k=3, H=128, I=256, split1=(128, 0, 0), split2=(0, 256, 0), wmode="w4", rounding="fused", bias="none"),
    "E": dict(E=5, k=1, H=128, I=384, split1=(0, 0, 128), split2=(128, 128, 128), wmode="w", rounding="reference", bias="none"),
}


def _ones_at(E, where):
    c = [0] * E
    for e in where:
        c[e] = 1
    return tuple(c)


# name -> (configuration, T, rows per expert); sum = T k and every count <= T
SCRIPTED = {
    "A largest 16": ("A", 24, (1, 16, 3, 0, 9, 0, 16, 3)),
    "A largest 32": ("A", 40, (32, 17, 0, 2, 9, 1, 16, 3)),
    "A largest 48": ("A", 60, (48, 33, 0, 7, 16, 1, 12, 3)),
    "A largest 64": ("A", 80, (64, 49, 0, 5, 17, 1, 21, 3)),
    "A mixed": ("A", 200, (0, 1, 16, 17, 64, 65, 129, 108)),
    # experts 0-7 all <= 64, two of them empty; experts 8-15 all > 64 but one with exactly 64
    "B two launches": ("B", 194, (0, 1, 16, 17, 0, 33, 64, 51, 65, 66, 64, 129, 65, 70, 67, 68)),
    "C one token": ("C", 1, _ones_at(64, (3, 9, 17, 26, 31, 40, 57, 63))),
    "D T=1": ("D", 1, (1, 1, 1)),
    "D T=7": ("D", 7, (7, 7, 7)),
    "D T=70": ("D", 70, (70, 70, 70)),
    "E k=1": ("E", 123, (0, 65, 1, 17, 40)),
}


def bias_layers(cfg, e):
    """which of (w1, w3, w2) of expert e carry a bias"""
    if cfg["bias"] == "odd experts":
        return (bool(e % 2),) * 3
    if cfg["bias"] == "w2":
        return (False, False, True)
    assert cfg["bias"] == "none"
    return (False, False, False)


# ---- scripted routing ---------------------------------------------------------------------------------------------------------------
def scripted_ids(counts, T, k):
    """int32 [T, k]: token t's experts in k-slot order, np.bincount of it = counts.  The experts, each repeated count times, are laid
    out in one row of T k entries; token t takes the entries t, t + T, t + 2 T, ... -- distinct experts, since no expert has more than
    T entries in a row -- and lists them from entry (t mod k) T + t on, so that the k-slot order is not always the expert order."""
    counts = np.asarray(counts, dtype=np.int64)
    if counts.sum() != T * k or (counts < 0).any() or counts.max() > T:
        raise ValueError("rows per expert must sum to T k and none may exceed T")
    seq = np.repeat(np.arange(len(counts)), counts).reshape(k, T)
    t = np.arange(T)
    ids = np.stack([seq[(j + t) % k, t] for j in range(k)], axis=1)
    assert all(len(set(row)) == k for row in ids.tolist())
    return ids.astype(np.int32)


def gate_unit_bits(E, H):
    """bf16 bits [E, H]: gate_weight[e] = the unit vector of column e"""
    assert E <= H
    g = np.zeros((E, H), dtype=np.float32)
    g[np.arange(E), np.arange(E)] = 1.0
    return o.f32_to_bf16(g)


def scripted_logit_bits(ids, E):
    """bf16 bits [T, E]: 4 * 2^-j on the expert of k-slot j, -4 elsewhere"""
    T, k = ids.shape
    l = np.full((T, E), -4.0, dtype=np.float32)
    l[np.arange(T)[:, None], ids] = (4.0 * 0.5 ** np.arange(k, dtype=np.float32))[None, :]
    return o.f32_to_bf16(l)


def scripted_x(counts, T, k, base_bits):
    """base_bits: uint16 [T, H] activations.  Returns (x bits with the routing values in the first E columns, the ids they force)."""
    E = len(counts)
    ids = scripted_ids(counts, T, k)
    x = np.array(base_bits, dtype=np.uint16, copy=True)
    assert x.shape[0] == T and x.shape[1] >= E and np.isfinite(o.bf16_to_f32(x)).all()
    x[:, :E] = scripted_logit_bits(ids, E)
    return x, ids


# ---- the oracle block ---------------------------------------------------------------------------------------------------------------
def f64_to_bf16_signed(x):
    """float64 -> bf16 bits, ONE rounding to nearest even: signs, zeros and the bf16 subnormals (quantum 2^-133) included"""
    x = np.asarray(x, dtype=np.float64)
    a = np.abs(x)
    _, e = np.frexp(a)                                         # a = m * 2^e, m in [0.5, 1)
    e = np.maximum(e, -125)                                    # below 2^-126 the quantum stays 2^-133
    q = np.ldexp(np.rint(np.ldexp(a, 8 - e)), e - 8)           # rint rounds halves to even
    v = np.copysign(q, x).astype(np.float32)                   # exact: at most 8 significant bits
    assert np.all(v.view(np.uint32) & np.uint32(0xFFFF) == 0)
    return (v.view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def silu_mul_bf16(a_bits, b_bits):
    """h = bf16(bf16(silu(a)) * b): silu in fp64 rounded once to bf16, then the product of two bf16 values (exact in fp32) rounded once
    -- what `F.silu(a) * b` on bf16 tensors means (qMixtralLayer.py:511)"""
    a = o.bf16_to_f32(a_bits).astype(np.float64)
    with np.errstate(over="ignore"):
        s = a / (1.0 + np.exp(-a))
    s = o.bf16_to_f32(f64_to_bf16_signed(s))
    return o.f32_to_bf16(s * o.bf16_to_f32(b_bits))


class OracleExpert:
    """one expert on the host: bf16 bits of w1, w3 [I, H] and w2 [H, I], their biases (or None), the two reorder indices; packs its
    weights with the oracle's quantizer when first asked"""

    def __init__(self, cfg, w_bits, bias_bits, idx1, idx2):
        self.cfg, self.w_bits, self.bias_bits = cfg, list(w_bits), list(bias_bits)
        self.idx = (np.asarray(idx1), np.asarray(idx1), np.asarray(idx2))
        self.split = (cfg["split1"], cfg["split1"], cfg["split2"])
        self._packed, self._deq = {}, {}

    def packed(self, i):
        if i not in self._packed:
            self._packed[i] = list(o.qlinear_pack_weight(self.w_bits[i], self.idx[i], *self.split[i], self.cfg["wmode"]))
        return self._packed[i]

    def deq(self, i):
        if i not in self._deq:
            self._deq[i] = o.dequant_operand(self.packed(i), "w", self.cfg["wmode"])
        return self._deq[i]

    def quantize(self, x_bits, i):
        return o.reorder_quantize(x_bits, self.idx[i], *self.split[i], "x")

    def linear(self, q, i):
        """layer i on the quantized rows q: the three-segment product, then y = bf16(y + bias)"""
        b = self.packed(i)
        y = o.matmul(q[0], b[0], q[1], b[1], q[2], b[2], q[3], b[3], q[4], b[4], q[5], b[5], rounding=self.cfg["rounding"], b_dequant=self.deq(i))
        if self.bias_bits[i] is not None:
            y = o.f32_to_bf16(o.bf16_to_f32(y) + o.bf16_to_f32(self.bias_bits[i])[None, :])
        return y

    def mlp(self, x_bits, act=silu_mul_bf16):
        q = self.quantize(x_bits, 0)                           # w1 and w3 read the same quantized rows
        h = act(self.linear(q, 0), self.linear(q, 1))
        return self.linear(self.quantize(h, 2), 2)


def gate_logit_bits(x_bits, gate_w_bits, gate_b_bits=None):
    """the gate linear in fp64, rounded once to bf16 (exact for scripted inputs)"""
    l = o.bf16_to_f32(x_bits).astype(np.float64) @ o.bf16_to_f32(gate_w_bits).astype(np.float64).T
    if gate_b_bits is not None:
        l = l + o.bf16_to_f32(gate_b_bits).astype(np.float64)[None, :]
    return f64_to_bf16_signed(l)


def oracle_block(x_bits, experts, top_k, logit_bits, act=silu_mul_bf16):
    """x bits [T, H], logits bits [T, E] -> dict(out bits [T, H], ids, w_bits, w (fp64, before its rounding), slot_of, offsets)"""
    E, H = len(experts), x_bits.shape[1]
    ids, w_bits, w = mo.route(logit_bits, top_k)
    offsets, sorted_token, slot_of = mo.plan(ids, E)
    xs = x_bits[sorted_token]
    y = np.zeros((len(sorted_token), H), dtype=np.uint16)
    for e in range(E):
        if offsets[e + 1] > offsets[e]:
            y[offsets[e]:offsets[e + 1]] = experts[e].mlp(xs[offsets[e]:offsets[e + 1]], act)
    return dict(out=mo.combine(y, ids, w_bits, slot_of), ids=ids, w_bits=w_bits, w=w, slot_of=slot_of, offsets=offsets, y=y)


def unquantized_block(x_bits, experts, ids, w):
    """float64 [T, H]: the routing (ids, w) through fp64 products of the bf16 weights, biases included, nothing quantized or rounded"""
    x = o.bf16_to_f32(x_bits).astype(np.float64)
    out = np.zeros(x.shape, dtype=np.float64)
    f = lambda bits: o.bf16_to_f32(bits).astype(np.float64)
    for e, ex in enumerate(experts):
        t, j = np.nonzero(ids == e)
        if len(t) == 0:
            continue
        lin = lambda v, i: v @ f(ex.w_bits[i]).T + (f(ex.bias_bits[i])[None, :] if ex.bias_bits[i] is not None else 0.0)
        a, b = lin(x[t], 0), lin(x[t], 1)
        out[t] += lin(a / (1.0 + np.exp(-a)) * b, 2) * w[t, j][:, None]
    return out


def relative_distance(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ---- drawing a block's tensors --------------------------------------------------------------------------------------------------------
def draw_experts(cfg, dev, seed=0):
    """every expert's own weights, biases and two reorder indices as torch tensors on `dev`, from the generators of tests/model_case.py
    (weights N(0, 0.08) as in tests/test_moe_gpu.py): a list of dict(w=(w1, w3, w2), bias=(b1, b3, b2), idx1, idx2)"""
    from model_case import gen_bf16, gen_index
    H, I = cfg["H"], cfg["I"]
    out = []
    for e in range(cfg["E"]):
        s = seed + 10 * e
        w = (gen_bf16(dev, I, H, s, "w") * 4, gen_bf16(dev, I, H, s + 1, "w") * 4, gen_bf16(dev, H, I, s + 2, "w") * 4)
        bias = tuple(gen_bf16(dev, 1, n, s + 3 + i, "x")[0] * 0.1 if has else None
                     for i, (n, has) in enumerate(zip((I, I, H), bias_layers(cfg, e))))
        out.append(dict(w=w, bias=bias, idx1=gen_index(dev, H, s + 6), idx2=gen_index(dev, I, s + 7)))
    return out


def oracle_experts(cfg, drawn):
    from conftest import bits_from_t, u8
    return [OracleExpert(cfg, [bits_from_t(w) for w in d["w"]], [bits_from_t(b) if b is not None else None for b in d["bias"]],
                         u8(d["idx1"]), u8(d["idx2"])) for d in drawn]
