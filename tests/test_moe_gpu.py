"""GPU tests of the sparse MoE block (mm_moe_route / _plan / _gather / _combine, mixedgemm.moe_*, micromix_amd.moe.SparseMoEBlock) against
tests/moe_oracle.py, which tests/test_moe_cpu.py holds to torch's CPU results, and of the whole block against the reference's
per-expert loop (model/qMixtralLayer.py:414-452) written with the ops this library had before."""
import os
import subprocess
import sys

import numpy as np
import pytest

import moe_oracle as mo
from conftest import bits_from_t, t_from_bits
from micromix_amd import mixedgemm
from oracle import mx_oracle as o

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def i32(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def host(t):
    return t.cpu().numpy()


# ---- route ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,k", mo.ROUTE_SHAPES)
def test_route_against_the_oracle(dev, E, k):
    """ids equal to the oracle's (the tie rule included), every weight within 1 bf16 ulp of the fp64 oracle, at most 1 % of the weights
    of this (E, k) -- over its T = 1, 5, 64, 257 and its inputs; a fraction needs a population -- different from it at all; two launches
    bit-equal"""
    differ = total = 0
    for T in mo.ROUTE_TOKENS:
        for name, bits in mo.route_inputs(E, k, T).items():
            logits = t_from_bits(bits, dev)
            ids, w = mixedgemm.moe_route(logits, k)
            ids2, w2 = mixedgemm.moe_route(logits, k)
            want_ids, want_w, _ = mo.route(bits, k)
            assert ids.dtype.is_floating_point is False and tuple(ids.shape) == (T, k) and tuple(w.shape) == (T, k)
            assert np.array_equal(host(ids), want_ids), (name, T)
            ulp = o.bf16_ulp_distance(bits_from_t(w), want_w)
            print(f"route E={E} k={k} T={T} {name}: max {ulp.max()} ulp, {int((ulp != 0).sum())} of {ulp.size} differ")
            assert ulp.max() <= 1, (name, T)
            if name == "equal":
                assert np.array_equal(host(ids), np.tile(np.arange(k), (T, 1))) and (ulp == 0).all()
            differ, total = differ + int((ulp != 0).sum()), total + ulp.size
            assert np.array_equal(host(ids), host(ids2)) and np.array_equal(bits_from_t(w), bits_from_t(w2))
    assert differ <= 0.01 * total, (differ, total)


@pytest.mark.parametrize("E,k", mo.ROUTE_EDGE_SHAPES)
def test_route_at_the_edges(dev, E, k):
    """moe_oracle.route_edge_inputs: a tie exactly at the k boundary among otherwise distinct logits (two and three experts, low, high
    and mixed indices, -0.0 against +0.0) -- the lower index wins; experts masked with -inf; rows with k - 1 finite logits, where the
    -inf pick has weight +0.0; weights down to e^-80.  ids equal to the oracle's, weights within 1 bf16 ulp, two launches bit-equal"""
    for T in mo.ROUTE_EDGE_TOKENS:
        for name, bits in mo.route_edge_inputs(E, k, T).items():
            logits = t_from_bits(bits, dev)
            ids, w = mixedgemm.moe_route(logits, k)
            ids2, w2 = mixedgemm.moe_route(logits, k)
            want_ids, want_w, _ = mo.route(bits, k)
            assert np.array_equal(host(ids), want_ids), (name, T)
            ulp = o.bf16_ulp_distance(bits_from_t(w), want_w)
            print(f"route edge E={E} k={k} T={T} {name}: max {ulp.max()} ulp, {int((ulp != 0).sum())} of {ulp.size} differ")
            assert ulp.max() <= 1, (name, T)
            if name == "k - 1 finite":
                assert (bits_from_t(w)[:, k - 1] == 0).all(), "the -inf pick must have weight +0.0"
                assert np.isinf(o.bf16_to_f32(bits)[np.arange(T), host(ids)[:, k - 1]]).all()
            assert np.array_equal(host(ids), host(ids2)) and np.array_equal(bits_from_t(w), bits_from_t(w2))


# ---- plan -------------------------------------------------------------------------------------------------------------------------
def plan_cases():
    rng = np.random.default_rng(7)
    cases = {}
    for E, k in mo.ROUTE_SHAPES:
        for T in (5, 257):
            cases[f"routed E={E} k={k} T={T}"] = (mo.route(mo.route_inputs(E, k, T)["scale 1"], k)[0], E)
    cases["every token to one expert"] = (np.full((100, 2), 3, dtype=np.int32), 8)
    cases["one expert never chosen"] = (np.array([0, 1, 2, 3, 4, 6, 7], dtype=np.int32)[rng.integers(0, 7, (333, 2))], 8)
    for n in (1, 63, 64, 65, 1025, 40001):
        cases[f"n = {n}"] = (rng.integers(0, 8, (n, 1)).astype(np.int32), 8)
    cases["n = 40000, E = 64, k = 8"] = (rng.integers(0, 64, (5000, 8)).astype(np.int32), 64)
    cases["n = 2^20 + 3"] = (rng.integers(0, 8, (2 ** 20 + 3, 1)).astype(np.int32), 8)      # 257 chunks
    for name, (T, k, E, where) in {"a few bad ids": (300, 2, 8, (0, 7, 300, 599)), "bad ids over chunks": (3000, 3, 5, (4095, 4096, 8191, 8999)),
                                   "only bad ids": (3, 2, 8, tuple(range(6)))}.items():
        ids = rng.integers(0, E, (T, k)).astype(np.int32)
        ids.reshape(-1)[list(where)] = [(-1, E)[i % 2] for i in range(len(where))]
        cases[name] = (ids, E)
    return cases


PLAN_CASES = plan_cases()


@pytest.mark.parametrize("name", list(PLAN_CASES))
def test_plan_against_the_oracle(dev, name):
    import torch
    ids, E = PLAN_CASES[name]
    T, k = ids.shape
    want = mo.plan(ids, E)
    d_ids = i32(ids, dev)
    outs = []
    for fill in (-7, 12345):                                  # whatever the outputs held: every entry is written
        given = dict(expert_offsets=torch.full((E + 1,), fill, dtype=torch.int32, device=dev),
                     sorted_token=torch.full((T * k,), fill, dtype=torch.int32, device=dev),
                     slot_of=torch.full((T, k), fill, dtype=torch.int32, device=dev))
        got = mixedgemm.moe_plan(d_ids, E, **given)
        assert all(g is given[n] for g, n in zip(got, ("expert_offsets", "sorted_token", "slot_of")))
        outs.append([host(t) for t in got])
    for what, g0, g1, w in zip(("expert_offsets", "sorted_token", "slot_of"), outs[0], outs[1], want):
        assert np.array_equal(g0, w), f"{name}: {what}"
        assert np.array_equal(g0, g1), f"{name}: {what} differs between two launches"
    alloc = mixedgemm.moe_plan(d_ids, E)                      # outputs allocated by the call
    assert all(np.array_equal(host(a), w) for a, w in zip(alloc, want))


def test_plan_without_tokens(dev):
    import torch
    off, tok, slot = mixedgemm.moe_plan(torch.empty((0, 2), dtype=torch.int32, device=dev), 8)
    assert host(off).tolist() == [0] * 9 and tok.numel() == 0 and tuple(slot.shape) == (0, 2)


# ---- gather -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", (8, 384, 4096, 6152))
def test_gather_is_an_index_copy(dev, H):
    """6152 = 8 * 769: three strides of 256 lanes and a tail; rows whose token lies outside [0, T) stay as they were"""
    import torch
    rng = np.random.default_rng(H)
    T, n = 37, 83
    x = t_from_bits(rng.integers(0, 1 << 16, (T, H)).astype(np.uint16), dev)     # any bit pattern: a copy
    tok = rng.integers(0, T, n).astype(np.int32)
    tok[[0, 41, n - 1]] = (T - 1, 0, T - 1)
    got = mixedgemm.moe_gather(x, i32(tok, dev))
    assert np.array_equal(bits_from_t(got), bits_from_t(x)[tok])
    tok[[3, 50, n - 2]] = (-1, T, 2 ** 31 - 1)
    before = t_from_bits(rng.integers(0, 1 << 16, (n, H)).astype(np.uint16), dev)
    want = bits_from_t(before).copy()
    keep = (tok >= 0) & (tok < T)
    want[keep] = bits_from_t(x)[tok[keep]]
    out = mixedgemm.moe_gather(x, i32(tok, dev), out=before)
    assert out is before and np.array_equal(bits_from_t(out), want)
    assert tuple(mixedgemm.moe_gather(x, i32(tok[:0], dev)).shape) == (0, H)
    with pytest.raises(RuntimeError):
        mixedgemm.moe_gather(torch.zeros((4, 12), dtype=torch.bfloat16, device=dev), i32([0], dev))     # H % 8


def test_operands_at_the_end_of_their_allocations(dev):
    """gather and combine with every operand ending where its own allocation ends (a child process, as tests/test_rope_append_gpu.py does)"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "moe_bounds_probe.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "done" in p.stdout, (p.stdout[-1500:], p.stderr[-1500:])
    cases = [l.split() for l in p.stdout.splitlines() if l.startswith("case")]
    assert len(cases) == 3
    for c in cases:
        assert c[-1] == c[-2], c            # the same bytes as with the operands in the middle of torch's pool


# ---- combine ----------------------------------------------------------------------------------------------------------------------
def run_combine(dev, y_bits, ids, w_bits, slot_of):
    """the kernel's result over an `out` filled with NaN: every row must be overwritten"""
    import torch
    T, H = ids.shape[0], y_bits.shape[1]
    out = torch.full((T, H), float("nan"), dtype=torch.bfloat16, device=dev)
    got = mixedgemm.moe_combine(t_from_bits(y_bits, dev), i32(ids, dev), t_from_bits(w_bits, dev), i32(slot_of, dev), out=out)
    assert got is out
    return bits_from_t(got)


@pytest.mark.parametrize("k,E,H", [(1, 8, 8), (2, 8, 384), (4, 16, 2056), (8, 8, 4096), (2, 64, 4096), (3, 5, 64), (5, 8, 72), (6, 6, 136), (7, 9, 200)])
def test_combine_against_the_oracle(dev, k, E, H):
    """Gaussian y, routed weights; then the same with a few entries (and one whole token) without a slot"""
    rng = np.random.default_rng(100 * k + E)
    T = 67
    ids, w_bits, _ = mo.route(o.f32_to_bf16(rng.standard_normal((T, E)).astype(np.float32)), k)
    slot_of = mo.plan(ids, E)[2]
    y = o.f32_to_bf16(rng.standard_normal((T * k, H)).astype(np.float32))
    assert np.array_equal(run_combine(dev, y, ids, w_bits, slot_of), mo.combine(y, ids, w_bits, slot_of))
    slot_of = slot_of.copy()
    slot_of[rng.integers(0, T, 9), rng.integers(0, k, 9)] = -1
    slot_of[11] = -1                                          # a token with no entry: zeros
    got = run_combine(dev, y, ids, w_bits, slot_of)
    assert np.array_equal(got, mo.combine(y, ids, w_bits, slot_of))
    assert (got[11] == 0).all()
    assert np.array_equal(bits_from_t(mixedgemm.moe_combine(t_from_bits(y, dev), i32(ids, dev), t_from_bits(w_bits, dev), i32(slot_of, dev))), got)


def test_combine_adds_in_ascending_expert_order(dev):
    """2^8, 1, 1, -2^8 on experts 0..3 with weight 1: ascending expert order gives 0 (256 + 1 rounds back to 256, twice), 1 + 1 first
    would give 2 -- in every order topk_ids can list the four"""
    import itertools
    perms = np.array(list(itertools.permutations(range(4))), dtype=np.int32)     # 24 tokens
    T = len(perms)
    slot_of = mo.plan(perms, 4)[2]
    vals = o.f32_to_bf16(np.array([256.0, 1.0, 1.0, -256.0], dtype=np.float32))
    y = np.repeat(np.repeat(vals, T)[:, None], 16, axis=1)    # expert e owns the slots [e T, (e + 1) T)
    w_bits = np.full((T, 4), 0x3F80, dtype=np.uint16)
    got = run_combine(dev, y, perms, w_bits, slot_of)
    assert np.array_equal(got, mo.combine(y, perms, w_bits, slot_of))
    assert (got == 0).all()


def test_combine_exact_ties(dev):
    """the products and sums of tests/test_moe_cpu.py that lie exactly between two bf16 values"""
    f = lambda *v: o.f32_to_bf16(np.array(v, dtype=np.float32))
    a, b = 1 + 2.0 ** -7, 1 + 3 * 2.0 ** -7
    ys = f(1.5, 256.0, 258.0, 3.0, 1.0, 1.0, -1.5, 3.0, -1.0, 1.5, -256.0, 5.0)
    ws = f(a, 1.0, 1.0, a, 1.0, 1.0, b, 1.0, 1.0, b, 1.0, a)
    ids = np.array([[3, 0, 2, 1], [1, 3, 0, 2], [0, 1, 2, 3]], dtype=np.int32)
    slot_of = mo.plan(ids, 4)[2]
    w_bits = ws[slot_of]
    y = np.repeat(ys[:, None], 8, axis=1)
    got = run_combine(dev, y, ids, w_bits, slot_of)
    assert np.array_equal(got, mo.combine(y, ids, w_bits, slot_of))
    assert o.bf16_to_f32(got[1:, 0]).tolist() == [4.0, 266.0]


# ---- matmul_grouped(outs=) ----------------------------------------------------------------------------------------------------------
def test_grouped_matmul_writes_into_given_outputs(dev):
    import torch
    g = torch.Generator().manual_seed(5)
    n, k, split, ms = 256, 256, (128, 0, 128), (3, 0, 70, 17)
    As, Bs = [], []
    for m in ms:
        idx = torch.randperm(k, generator=g).to(torch.int16).to(dev)
        Bs.append(mixedgemm.reorder_quantize_w4((torch.randn((n, k), generator=g) * 0.05).to(torch.bfloat16).to(dev), idx, *split))
        As.append(mixedgemm.reorder_quantize_x(torch.randn((m, k), generator=g).to(torch.bfloat16).to(dev), idx, *split))
    want = mixedgemm.matmul_grouped(As, Bs)
    buf = torch.full((sum(ms) + 2, n), float("nan"), dtype=torch.bfloat16, device=dev)
    edges = np.concatenate([[0], np.cumsum(ms)]) + 1          # a guard row on either side
    outs = [buf[edges[i]:edges[i + 1]] for i in range(len(ms))]
    got = mixedgemm.matmul_grouped(As, Bs, outs=outs)
    assert all(a is b for a, b in zip(got, outs))
    assert torch.equal(buf[1:-1], torch.cat(want)) and bool(buf[0].isnan().all()) and bool(buf[-1].isnan().all())
    with pytest.raises(RuntimeError):
        mixedgemm.matmul_grouped(As, Bs, outs=[buf[: m + 1] for m in ms])       # wrong shapes
    with pytest.raises(ValueError):
        mixedgemm.matmul_grouped(As, Bs, outs=outs[:2])


# ---- the block ----------------------------------------------------------------------------------------------------------------------
E_BLOCK, K_BLOCK, H_BLOCK, SPLIT = 8, 2, 384, (128, 128, 128)


@pytest.fixture(scope="module")
def experts(dev):
    """eight experts, H = I = 384, split (128, 128, 128), every expert with its own weights and reorder indices; packed with
    reorder_quantize_w4 (QLinearLayer's default) from the generators of tests/model_case.py"""
    import torch
    from micromix_amd.qlinear import QLinearLayer
    from model_case import gen_bf16, gen_index

    def layer(seed, index):
        lin = torch.nn.Linear(H_BLOCK, H_BLOCK, bias=False, dtype=torch.bfloat16, device=dev)
        lin.weight.data = gen_bf16(dev, H_BLOCK, H_BLOCK, seed, "w") * 4          # N(0, 0.08): outputs of the order of the inputs
        return QLinearLayer(lin, p8_num=SPLIT[2], p6_num=SPLIT[1], reorder_index=index)

    out = []
    for e in range(E_BLOCK):
        i1, i2 = gen_index(dev, H_BLOCK, 50 + e), gen_index(dev, H_BLOCK, 70 + e)
        out.append((layer(3 * e, i1), layer(3 * e + 1, i1), layer(3 * e + 2, i2)))
    return out


def reference_loop(x, gate_w, gate_b, experts, top_k):
    """MixtralSparseMoeBlock.forward as the reference runs it (qMixtralLayer.py:414-452, 502-519), expert by expert, with the routing
    that moe_route returned: torch.where, index copy, reorder_quantize_x, matmul (split_k=False as in tests/test_grouped_gpu.py: the
    grouped launches never split K), F.silu(a) * b, reorder_quantize_x, matmul, * w, index_add_"""
    import torch
    import torch.nn.functional as F
    mm = lambda q, l: mixedgemm.matmul(q[0], l.BN, q[1], l.BS, q[2], l.BO, q[3], l.SFBN, q[4], l.SFBS, q[5], l.SFBO, split_k=False)
    logits = F.linear(x, gate_w, gate_b)
    ids, w = mixedgemm.moe_route(logits, top_k)
    final = torch.zeros_like(x)
    mask = torch.nn.functional.one_hot(ids.long(), num_classes=len(experts)).permute(2, 1, 0)
    for e, (w1, w3, w2) in enumerate(experts):
        idx, top_x = torch.where(mask[e])
        if top_x.numel() == 0:
            continue
        cur = x[None, top_x].reshape(-1, x.size(1))
        q = mixedgemm.reorder_quantize_x(cur, w1.reorder_index, w1.p4_num, w1.p6_num, w1.p8_num)
        h = F.silu(mm(q, w1)) * mm(q, w3)
        q = mixedgemm.reorder_quantize_x(h, w2.reorder_index, w2.p4_num, w2.p6_num, w2.p8_num)
        cur = mm(q, w2) * w[top_x, idx, None]
        final.index_add_(0, top_x, cur)
    return final, logits, ids


@pytest.mark.parametrize("bias", (False, True))
@pytest.mark.parametrize("T", (1, 7, 64, 300))
def test_block_equals_the_reference_loop(dev, experts, T, bias):
    import torch
    from micromix_amd import SparseMoEBlock
    from model_case import gen_bf16
    g = torch.Generator().manual_seed(T)
    gate_w = (torch.randn((E_BLOCK, H_BLOCK), generator=g) * 0.05).to(torch.bfloat16).to(dev)
    gate_b = None
    if bias:                                                  # experts 2 and 5 are never chosen: two groups with M = 0
        gate_b = torch.zeros((E_BLOCK,), dtype=torch.bfloat16, device=dev)
        gate_b[[2, 5]] = -1000.0
    block = SparseMoEBlock(gate_w, experts, K_BLOCK, gate_bias=gate_b)
    x = gen_bf16(dev, T, H_BLOCK, 900 + T, "x")
    out, logits = block(x.reshape(1, T, H_BLOCK))
    want, want_logits, ids = reference_loop(x, gate_w, gate_b, experts, K_BLOCK)
    torch.cuda.synchronize()
    counts = np.bincount(host(ids).reshape(-1), minlength=E_BLOCK)
    if bias:
        assert counts[2] == 0 and counts[5] == 0
    print(f"block T={T} bias={bias}: rows per expert {counts.tolist()}")
    if T == 300:
        assert counts.max() > 64                              # 600 pairs over 8 experts: the tiled grouped launch takes part too
    assert tuple(out.shape) == (1, T, H_BLOCK) and tuple(logits.shape) == (T, E_BLOCK)
    assert torch.equal(logits, want_logits)
    assert bool(torch.isfinite(want).all()) and float(want.float().abs().max()) > 0
    assert torch.equal(out.reshape(T, H_BLOCK), want)
    out2, _ = block(x)                                        # 2-D input, a second launch: the same bits
    assert torch.equal(out2, want)


def test_block_accepts_expert_objects_and_rejects_mismatches(dev, experts):
    import types
    import torch
    from micromix_amd import SparseMoEBlock
    gate = torch.nn.Linear(H_BLOCK, E_BLOCK, bias=True, dtype=torch.bfloat16, device=dev)
    objs = [types.SimpleNamespace(w1=a, w3=b, w2=c) for a, b, c in experts]
    block = SparseMoEBlock(gate, objs, K_BLOCK)
    x = torch.randn((9, H_BLOCK), device=dev).to(torch.bfloat16)
    out, logits = block(x)
    want, want_logits, _ = reference_loop(x, gate.weight.data, gate.bias.data, experts, K_BLOCK)
    assert torch.equal(out, want) and torch.equal(logits, want_logits)
    empty, _ = block(x[:0])
    assert tuple(empty.shape) == (0, H_BLOCK)
    with pytest.raises(ValueError):
        SparseMoEBlock(gate, [(a, c, c) for a, b, c in experts], K_BLOCK)     # w3 with another reorder index than w1
    with pytest.raises(ValueError):
        SparseMoEBlock(gate, objs, 9)
