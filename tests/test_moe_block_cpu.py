"""CPU tests of tests/moe_block_oracle.py: the scripted-routing builder produces the rows per expert it is asked for, through a real bf16
gate linear, for every count vector the GPU tests use; and the numpy oracle block is the reference's per-expert loop
(model/qMixtralLayer.py:414-452, 502-519) on the CPU, bit for bit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import moe_block_oracle as mb
import moe_oracle as mo
from conftest import bits_from_t, make_inputs, t_from_bits
from oracle import mx_oracle as o


@pytest.mark.parametrize("name", list(mb.SCRIPTED))
def test_builder_forces_the_scripted_rows_per_expert(name):
    cfg_id, T, counts = mb.SCRIPTED[name]
    cfg = mb.CONFIGS[cfg_id]
    E, k, H = cfg["E"], cfg["k"], cfg["H"]
    assert len(counts) == E and sum(counts) == T * k and max(counts) <= T
    x, ids = mb.scripted_x(counts, T, k, make_inputs(np.random.default_rng(T), T, H))
    assert np.array_equal(np.bincount(ids.reshape(-1), minlength=E), counts)
    assert all(len(set(row)) == k for row in ids.tolist())
    want = mb.scripted_logit_bits(ids, E)
    assert np.array_equal(mb.gate_logit_bits(x, mb.gate_unit_bits(E, H)), want)
    # a real bf16 linear: every product is a power of two or zero, so the sum is exact in any order
    logits = F.linear(t_from_bits(x, "cpu"), t_from_bits(mb.gate_unit_bits(E, H), "cpu"))
    assert np.array_equal(bits_from_t(logits), want)
    got_ids, w_bits, _ = mo.route(want, k)
    assert np.array_equal(got_ids, ids)
    assert np.array_equal(x[:, E:], make_inputs(np.random.default_rng(T), T, H)[:, E:])       # the other columns are the activations
    if k > 1 and T >= k:
        assert any(row != sorted(row) for row in ids.tolist())       # the k-slot order is not always the expert order


def test_builder_covers_what_the_issue_lists():
    """the four streaming tiers, the 64 / 65 boundary, a group past 128 rows, empty groups, E = 16 and 64"""
    a = {n: c for n, (cfg, _, c) in mb.SCRIPTED.items() if cfg == "A"}
    small_max = sorted(max(v for v in c if v <= 64) for n, c in a.items() if n != "A mixed")
    assert [(m - 1) // 16 for m in small_max] == [0, 1, 2, 3]
    mixed = a["A mixed"]
    assert {0, 1, 16, 17, 64, 65}.issubset(mixed) and max(mixed) > 128
    b = mb.SCRIPTED["B two launches"][2]
    assert len(b) == 16 and max(b[:8]) <= 64 and b[:8].count(0) == 2 and sorted(b[8:])[0] == 64 and sorted(b[8:])[1] > 64
    assert sum(1 for v in mb.SCRIPTED["C one token"][2] if v == 0) == 56
    e = mb.SCRIPTED["E k=1"][2]
    assert 0 in e and 65 in e
    with pytest.raises(ValueError):
        mb.scripted_ids((3, 1), 2, 2)                         # an expert with more rows than there are tokens
    with pytest.raises(ValueError):
        mb.scripted_ids((1, 1), 2, 2)                         # not T k rows


TINY = dict(E=4, k=2, H=128, I=256, split1=(0, 0, 128), split2=(128, 0, 128), wmode="w4", rounding="reference", bias="odd experts")


def torch_act(a_bits, b_bits):
    return bits_from_t(F.silu(t_from_bits(a_bits, "cpu")) * t_from_bits(b_bits, "cpu"))


def reference_loop_cpu(x_bits, experts, logit_bits, top_k):
    """the reference's loop with o.qlinear_forward for the layers and torch's CPU bf16 for everything between them; the routing is
    the oracle's (torch.topk leaves ties open; tests/test_moe_cpu.py holds the two together).  Returns the output bits and every
    (a, b) pair that went into the activation."""
    ids, w_bits, _ = mo.route(logit_bits, top_k)
    x, w = t_from_bits(x_bits, "cpu"), t_from_bits(w_bits, "cpu")
    final = torch.zeros_like(x)
    mask = F.one_hot(torch.from_numpy(ids.astype(np.int64)), num_classes=len(experts)).permute(2, 1, 0)
    acts = []
    for e, ex in enumerate(experts):
        idx, top_x = torch.where(mask[e])
        if top_x.numel() == 0:
            continue
        lin = lambda bits, i: o.qlinear_forward(bits, ex.idx[i], *ex.split[i], ex.packed(i), bias_bits=ex.bias_bits[i], rounding=ex.cfg["rounding"])
        cur = bits_from_t(x[None, top_x].reshape(-1, x.size(1)))
        a, b = lin(cur, 0), lin(cur, 1)
        acts.append((a, b))
        h = F.silu(t_from_bits(a, "cpu")) * t_from_bits(b, "cpu")
        cur = t_from_bits(lin(bits_from_t(h), 2), "cpu") * w[top_x, idx, None]
        final.index_add_(0, top_x, cur)
    return bits_from_t(final), acts


@pytest.mark.parametrize("routing", ("scripted", "gaussian"))
def test_oracle_block_is_the_reference_loop_on_the_cpu(routing):
    """Bit for bit, with one proviso.  The oracle's activation rounds silu(a), evaluated in fp64, once to bf16; torch's CPU kernel
    evaluates a / (1 + exp(-a)) in fp32 first, which is not correctly rounded for every input, so a rare h differs in its last bit
    and everything after it follows.  Hence: the activation stage alone is held to the 2-ulp bound of the GPU test (one ulp per
    rounding) and its share of unequal results is printed; the block is compared with the loop bit for bit when both run on torch's
    activation; and where torch's h equals the oracle's on every drawn input -- checked, not assumed -- the oracle block with its own
    activation is the loop bit for bit too."""
    cfg = TINY
    E, k, H, T = cfg["E"], cfg["k"], cfg["H"], 37
    experts = mb.oracle_experts(cfg, mb.draw_experts(cfg, "cpu", seed=400))
    assert [e.bias_bits[0] is not None for e in experts] == [False, True, False, True]
    base = make_inputs(np.random.default_rng(5), T, H)
    if routing == "scripted":
        counts = (30, 0, 37, 7)
        x, ids = mb.scripted_x(counts, T, k, base)
        logits = bits_from_t(F.linear(t_from_bits(x, "cpu"), t_from_bits(mb.gate_unit_bits(E, H), "cpu")))
    else:
        x = base
        gate = o.f32_to_bf16((0.05 * np.random.default_rng(6).standard_normal((E, H))).astype(np.float32))
        logits = bits_from_t(F.linear(t_from_bits(x, "cpu"), t_from_bits(gate, "cpu")))
    want, acts = reference_loop_cpu(x, experts, logits, k)
    got = mb.oracle_block(x, experts, k, logits, act=torch_act)
    if routing == "scripted":
        assert np.array_equal(got["ids"], ids) and np.array_equal(np.bincount(got["ids"].reshape(-1), minlength=E), counts)
    assert np.isfinite(o.bf16_to_f32(want)).all() and np.abs(o.bf16_to_f32(want)).max() > 0
    assert np.array_equal(got["out"], want)
    unequal = total = 0
    for a, b in acts:
        ulp = o.bf16_ulp_distance(torch_act(a, b), mb.silu_mul_bf16(a, b))
        assert ulp.max() <= 2
        unequal, total = unequal + int((ulp != 0).sum()), total + ulp.size
    print(f"oracle block, {routing}: torch's CPU silu(a) * b differs from the two-rounding fp64 expression in {unequal} of {total}")
    if unequal == 0:
        assert np.array_equal(mb.oracle_block(x, experts, k, logits)["out"], want)


def test_signed_rounding_helper():
    x = np.array([0.0, -0.0, 1.0, -1.0 - 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1.0 / 3.0, 2.0 ** -133, -(2.0 ** -134), 3 * 2.0 ** -134, 2.0 ** -126])
    want = np.array([0x0000, 0x8000, 0x3F80, 0xBF80, 0x3F82, 0xBEAB, 0x0001, 0x8000, 0x0002, 0x0080], dtype=np.uint16)
    assert np.array_equal(mb.f64_to_bf16_signed(x), want)
    pos = np.abs(np.random.default_rng(0).standard_normal(1000)) + 1e-3
    assert np.array_equal(mb.f64_to_bf16_signed(pos), mo.f64_to_bf16(pos))
    assert np.array_equal(mb.f64_to_bf16_signed(-pos), mo.f64_to_bf16(pos) | 0x8000)


def test_unquantized_block_is_a_plain_fp64_loop():
    cfg = TINY
    experts = mb.oracle_experts(cfg, mb.draw_experts(cfg, "cpu", seed=400))
    x, ids = mb.scripted_x((3, 0, 5, 2), 5, 2, make_inputs(np.random.default_rng(1), 5, cfg["H"]))
    _, _, w = mo.route(mb.scripted_logit_bits(ids, cfg["E"]), 2)
    got = mb.unquantized_block(x, experts, ids, w)
    f = lambda b: o.bf16_to_f32(b).astype(np.float64)
    for t in range(5):
        want = np.zeros(cfg["H"])
        for j in range(2):
            ex = experts[ids[t, j]]
            bias = [f(b) if b is not None else 0.0 for b in ex.bias_bits]
            a, b = f(ex.w_bits[0]) @ f(x[t]) + bias[0], f(ex.w_bits[1]) @ f(x[t]) + bias[1]
            want += w[t, j] * (f(ex.w_bits[2]) @ (a / (1 + np.exp(-a)) * b) + bias[2])
        assert np.allclose(got[t], want, rtol=1e-12, atol=1e-12)
