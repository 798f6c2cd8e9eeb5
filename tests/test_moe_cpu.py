"""CPU tests of the sparse-MoE oracle (tests/moe_oracle.py) and of the host side of the mm_moe_* entries: the oracle's combine is torch's
CPU bf16 zeros + per-expert index_add_ loop bit for bit, its plan is a stable argsort, its routing selects what torch.topk selects and
weighs within 1 bf16 ulp of torch's softmax -> topk -> renormalise -> cast; the entries' status codes come without device work."""
import numpy as np
import pytest
import torch

import moe_oracle as mo
from conftest import bits_from_t, t_from_bits
from micromix_amd import _lib
from oracle import mx_oracle as o


def torch_combine(y_bits, ids, w_bits, slot_of):
    """the reference's accumulation (qMixtralLayer.py:428-450) on the CPU, in bf16: zeros, then expert by expert index_add_ of y * w"""
    y, w = t_from_bits(y_bits, "cpu"), t_from_bits(w_bits, "cpu")
    T, k = ids.shape
    out = torch.zeros((T, y.shape[1]), dtype=torch.bfloat16)
    for e in sorted(set(int(i) for i in ids.reshape(-1))):
        for j in range(k):                                    # a routed token meets an expert once; the k-slot order covers the rest
            top_x = np.flatnonzero((ids[:, j] == e) & (slot_of[:, j] >= 0))
            if len(top_x):
                rows = torch.from_numpy(slot_of[top_x, j].astype(np.int64))
                cur = y[rows] * w[torch.from_numpy(top_x), j, None]
                out.index_add_(0, torch.from_numpy(top_x), cur)
    return bits_from_t(out)


def routed_case(rng, T, E, k, H, scale=1.0):
    logits = o.f32_to_bf16(rng.standard_normal((T, E)).astype(np.float32))
    ids, w_bits, _ = mo.route(logits, k)
    _, _, slot_of = mo.plan(ids, E)
    y = o.f32_to_bf16((scale * rng.standard_normal((T * k, H))).astype(np.float32))
    return y, ids, w_bits, slot_of


@pytest.mark.parametrize("T,E,k,H", [(37, 8, 2, 64), (20, 8, 1, 8), (33, 4, 4, 40), (25, 16, 8, 24)])
def test_combine_oracle_is_torch_index_add(T, E, k, H):
    rng = np.random.default_rng(T + k)
    y, ids, w_bits, slot_of = routed_case(rng, T, E, k, H)
    slot_of = slot_of.copy()
    slot_of[rng.integers(0, T, 3), rng.integers(0, k, 3)] = -1          # skipped entries
    assert np.array_equal(mo.combine(y, ids, w_bits, slot_of), torch_combine(y, ids, w_bits, slot_of))


def test_combine_oracle_exact_ties_in_both_roundings():
    """products that lie exactly half way between two bf16 values (token 0: 1.5 * (1 + 2^-7) = 1.5 + 2^-7 + 2^-8, and its like with
    an odd and an even lower neighbour and a negative sign) and sums that do (tokens 1 and 2: 256 + 1, 256 + 3, 258 + 1, 260 - 1; one
    bf16 ulp there is 2), in a k-slot order that is not the expert order.  Slot s = 3 e + t belongs to expert e, token t."""
    f = lambda *v: o.f32_to_bf16(np.array(v, dtype=np.float32))
    a, b = 1 + 2.0 ** -7, 1 + 3 * 2.0 ** -7
    #      e0: t0, t1, t2      e1              e2              e3
    ys = f(1.5, 256.0, 258.0,  3.0, 1.0, 1.0,  -1.5, 3.0, -1.0,  1.5, -256.0, 5.0)
    ws = f(a, 1.0, 1.0,        a, 1.0, 1.0,    b, 1.0, 1.0,      b, 1.0, a)
    T, k, H = 3, 4, 8
    y = np.repeat(ys[:, None], H, axis=1)                     # slot s holds ys[s] in every column
    ids = np.array([[3, 0, 2, 1], [1, 3, 0, 2], [0, 1, 2, 3]], dtype=np.int32)
    _, _, slot_of = mo.plan(ids, 4)
    w_bits = ws[slot_of]                                      # the weight of the pair in slot s is ws[s]
    got = mo.combine(y, ids, w_bits, slot_of)
    assert np.array_equal(got, torch_combine(y, ids, w_bits, slot_of))
    prod = o.bf16_to_f32(ys) * o.bf16_to_f32(ws)
    assert ((prod.view(np.uint32) & np.uint32(0xFFFF)) == 0x8000).sum() == 4       # token 0's four products are exact ties
    # 256 + 1 -> 256, + 3 -> 260, - 256 -> 4;  258 + 1 -> 260, - 1 -> 260, + bf16(5 (1 + 2^-7)) = 265.03 -> 266
    assert o.bf16_to_f32(got[1:, 0]).tolist() == [4.0, 266.0]


def test_combine_oracle_takes_ascending_expert_order():
    """2^8, 1, 1, -2^8 on experts 0..3: ascending order gives bf16(bf16(256 + 1) + 1) - 256 = 0 (256 + 1 ties to even, 256);
    another order gives 2 (1 + 1 first) -- whatever order topk_ids lists the four in"""
    vals = np.array([256.0, 1.0, 1.0, -256.0], dtype=np.float32)
    for perm in ([0, 1, 2, 3], [3, 2, 1, 0], [1, 2, 0, 3], [2, 0, 3, 1]):
        ids = np.array([perm], dtype=np.int32)
        _, _, slot_of = mo.plan(ids, 4)
        y = np.repeat(o.f32_to_bf16(vals)[:, None], 8, axis=1)          # slot e (one token: slot = expert) holds vals[e]
        w_bits = np.full((1, 4), 0x3F80, dtype=np.uint16)
        got = mo.combine(y, ids, w_bits, slot_of)
        assert np.array_equal(got, torch_combine(y, ids, w_bits, slot_of))
        assert (o.bf16_to_f32(got) == 0.0).all()
    assert float(torch.tensor(1.0, dtype=torch.bfloat16) + torch.tensor(1.0, dtype=torch.bfloat16) + torch.tensor(256.0, dtype=torch.bfloat16)
                 - torch.tensor(256.0, dtype=torch.bfloat16)) == 2.0      # the order matters


@pytest.mark.parametrize("T,E,k", [(1, 8, 2), (50, 8, 2), (33, 3, 2), (40, 64, 8), (4097, 8, 1)])
def test_plan_oracle_is_a_stable_argsort(T, E, k):
    rng = np.random.default_rng(T + E)
    ids = rng.integers(0, E, (T, k)).astype(np.int32)
    offsets, sorted_token, slot_of = mo.plan(ids, E)
    order = np.argsort(ids.reshape(-1), kind="stable")
    assert np.array_equal(sorted_token, order // k)
    assert np.array_equal(slot_of.reshape(-1)[order], np.arange(T * k))
    assert np.array_equal(offsets, np.searchsorted(ids.reshape(-1)[order], np.arange(E + 1)))
    for e in range(E):                                        # within an expert the slots run by ascending token
        assert (np.diff(sorted_token[offsets[e]:offsets[e + 1]]) >= 0).all()
    # ids outside [0, E): uncounted, slot_of = -1, the others as a sort of the valid pairs alone has them
    bad = ids.copy()
    bad.reshape(-1)[rng.integers(0, T * k, 3)] = (-1, E, -1)
    offsets, sorted_token, slot_of = mo.plan(bad, E)
    valid = np.flatnonzero((bad.reshape(-1) >= 0) & (bad.reshape(-1) < E))
    assert offsets[E] == len(valid) and (sorted_token[len(valid):] == -1).all()
    assert (slot_of.reshape(-1)[(bad.reshape(-1) < 0) | (bad.reshape(-1) >= E)] == -1).all()
    assert np.array_equal(sorted_token[: len(valid)], valid[np.argsort(bad.reshape(-1)[valid], kind="stable")] // k)


@pytest.mark.parametrize("E,k", mo.ROUTE_SHAPES)
def test_route_oracle_against_torch(E, k):
    for T in mo.ROUTE_TOKENS:
        for name, bits in mo.route_inputs(E, k, T).items():
            ids, w_bits, _ = mo.route(bits, k)
            if name == "equal":                               # the tie rule: ids 0..k-1, equal weights
                assert np.array_equal(ids, np.tile(np.arange(k, dtype=np.int32), (T, 1))), name
                assert np.array_equal(w_bits, np.full((T, k), mo.f64_to_bf16(1.0 / k), dtype=np.uint16)), name
                continue
            s = -np.sort(-o.bf16_to_f32(bits), axis=1)
            if k < E:
                assert (s[:, k - 1] != s[:, k]).all(), f"{name}: the generator's no-tie precondition"
            logits = t_from_bits(bits, "cpu")
            p = torch.softmax(logits, dim=1, dtype=torch.float)
            tw, ti = torch.topk(p, k, dim=-1)
            tw = (tw / tw.sum(dim=-1, keepdim=True)).to(torch.bfloat16)
            assert np.array_equal(np.sort(ids, axis=1), np.sort(ti.numpy(), axis=1)), f"{name}: top-k set"
            # torch's weights, brought into the oracle's order (ties inside the top k may be listed in another order)
            want = np.zeros((T, E), dtype=np.uint16)
            np.put_along_axis(want, ti.numpy(), bits_from_t(tw), axis=1)
            ulp = o.bf16_ulp_distance(w_bits, np.take_along_axis(want, ids.astype(np.int64), axis=1))
            assert ulp.max() <= 1, f"{name}: torch's CPU chain is {ulp.max()} bf16 ulps from the oracle"
            assert (ulp != 0).mean() <= 0.01, f"{name}: {(ulp != 0).mean():.4f} of torch's weights differ from the oracle"


def test_f64_to_bf16_rounds_once():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, 0.5, 1.0 / 3.0, 2.0 ** -30])
    want = np.array([0x3F80, 0x3F80, 0x3F82, 0x3F81, 0x3F00, 0x3EAB, 0x3080], dtype=np.uint16)
    assert np.array_equal(mo.f64_to_bf16(x), want)


def test_moe_status_codes_without_device_work():
    lib = _lib.load()
    z, p = None, 16                                           # p: a non-null, 16-byte aligned pointer that is never dereferenced here
    assert lib.mm_version() >= 630
    U, B, OK = _lib.MM_ERR_UNSUPPORTED, _lib.MM_ERR_BAD_ARG, _lib.MM_OK
    for E, k in ((8, 0), (8, 9), (2, 3), (65, 2), (0, 0)):
        assert lib.mm_moe_route(p, 4, E, k, p, p, z) == U, (E, k)
        assert lib.mm_moe_plan(p, 4, E, k, p, p, p, z) == U, (E, k)
    assert lib.mm_moe_combine(p, p, p, p, 4, 0, 64, p, z) == U and lib.mm_moe_combine(p, p, p, p, 4, 9, 64, p, z) == U
    assert lib.mm_moe_combine(p, p, p, p, 4, 2, 60, p, z) == U and lib.mm_moe_gather(p, p, 4, 8, 60, p, z) == U       # H % 8
    assert lib.mm_moe_route(p, 2 ** 30, 8, 8, p, p, z) == U                                                        # T * top_k >= 2^31
    assert lib.mm_moe_route(p, -1, 8, 2, p, p, z) == B and lib.mm_moe_plan(p, -1, 8, 2, p, p, p, z) == B
    assert lib.mm_moe_route(p, 4, 8, -2, p, p, z) == B and lib.mm_moe_plan(p, 4, -8, 2, p, p, p, z) == B
    assert lib.mm_moe_gather(p, p, -1, 8, 64, p, z) == B and lib.mm_moe_gather(p, p, 4, -8, 64, p, z) == B
    assert lib.mm_moe_gather(p, p, 4, 8, -64, p, z) == B and lib.mm_moe_combine(p, p, p, p, -4, 2, 64, p, z) == B
    # T = 0 (no rows): MM_OK, whatever the pointers
    assert lib.mm_moe_route(z, 0, 8, 2, z, z, z) == OK and lib.mm_moe_plan(z, 0, 8, 2, z, z, z, z) == OK
    assert lib.mm_moe_gather(z, z, 0, 8, 64, z, z) == OK and lib.mm_moe_gather(z, z, 4, 0, 64, z, z) == OK
    assert lib.mm_moe_combine(z, z, z, z, 0, 2, 64, z, z) == OK
    # null pointers, and bf16 rows that are not 16-byte aligned
    assert lib.mm_moe_route(z, 4, 8, 2, p, p, z) == B and lib.mm_moe_route(p, 4, 8, 2, z, p, z) == B and lib.mm_moe_route(p, 4, 8, 2, p, z, z) == B
    for i in range(4):
        a = [p] * 4
        a[i] = z
        assert lib.mm_moe_plan(a[0], 4, 8, 2, a[1], a[2], a[3], z) == B
        assert lib.mm_moe_combine(*a, 4, 2, 64, p, z) == B
    assert lib.mm_moe_combine(p, p, p, p, 4, 2, 64, z, z) == B and lib.mm_moe_combine(p, p, p, p, 4, 2, 64, 8, z) == B
    assert lib.mm_moe_gather(z, p, 4, 8, 64, p, z) == B and lib.mm_moe_gather(p, z, 4, 8, 64, p, z) == B
    assert lib.mm_moe_gather(p, p, 4, 8, 64, z, z) == B and lib.mm_moe_gather(8, p, 4, 8, 64, p, z) == B


# ---- the edges of the routing rule (moe_oracle.route_edge_inputs) ---------------------------------------------------------------------
def topk_set_is_unambiguous(bits, k):
    """rows whose k-th and (k + 1)-th largest logits differ: there torch.topk has one possible set"""
    s = -np.sort(-o.bf16_to_f32(bits).astype(np.float64), axis=1)
    return s[:, k - 1] != s[:, k]


@pytest.mark.parametrize("E,k", mo.ROUTE_EDGE_SHAPES)
def test_route_oracle_at_the_edges(E, k):
    """what the edge inputs are built to hold, in the oracle's own answer: at a tie the lower index wins (-0.0 = +0.0), a -inf expert is
    picked only when fewer than k are finite, then the lowest such index with weight +0.0, and the far weights are normal bf16 numbers;
    wherever the top-k set is unambiguous it is torch.topk's, with weights within 1 bf16 ulp of torch's chain"""
    for T in mo.ROUTE_EDGE_TOKENS:
        inputs = mo.route_edge_inputs(E, k, T)
        assert list(inputs) == ["tie of 2 at k", "tie of 3 at k", "masked", "k - 1 finite", "far"]
        for name, bits in inputs.items():
            l = o.bf16_to_f32(bits).astype(np.float64)
            assert bits.shape == (T, E) and not np.isnan(l).any()
            ids, w_bits, w = mo.route(bits, k)
            sel = np.take_along_axis(l, ids.astype(np.int64), axis=1)
            assert (np.diff(sel, axis=1) <= 0).all() and all(len(set(r)) == k for r in ids.tolist()), name
            if name.startswith("tie"):
                n = int(name.split()[2])
                zeros = 0
                for t in range(T):
                    tied = np.flatnonzero(l[t] == sel[t, k - 1])
                    assert len(tied) == n and (l[t] > sel[t, k - 1]).sum() < k <= (l[t] >= sel[t, k - 1]).sum() - 1
                    took = np.intersect1d(ids[t], tied)
                    assert np.array_equal(took, tied[: len(took)]), (name, t)          # the lowest indices among the tied
                    zeros += int(len(set(np.signbit(l[t, tied]).tolist())) == 2)
                assert zeros >= T // 3, name                  # rows where -0.0 meets +0.0
                assert not topk_set_is_unambiguous(bits, k).any()
            if name == "masked":
                assert np.isfinite(sel).all() and all(1 <= c <= E - k for c in np.isinf(l).sum(axis=1)), name
            if name == "k - 1 finite":
                assert (np.isfinite(l).sum(axis=1) == k - 1).all() and np.isfinite(sel[:, : k - 1]).all()
                assert np.array_equal(ids[:, k - 1], np.argmax(np.isinf(l), axis=1))       # the first -inf expert
                assert (w_bits[:, k - 1] == 0).all() and (w[:, k - 1] == 0).all()
            if name == "far":
                gaps = sel[:, :1] - sel[:, 1:]
                assert set(np.unique(gaps).tolist()) <= set(mo.FAR_GAPS) and gaps.max() == 80.0 and gaps.min() == 20.0
                assert (w > 2.0 ** -126).all() and ((w_bits & 0x7F80) != 0).all()         # normal bf16 numbers
            clear = topk_set_is_unambiguous(bits, k)
            if not clear.any():
                continue
            p = torch.softmax(t_from_bits(bits[clear], "cpu"), dim=1, dtype=torch.float)
            tw, ti = torch.topk(p, k, dim=-1)
            tw = (tw / tw.sum(dim=-1, keepdim=True)).to(torch.bfloat16)
            assert np.array_equal(np.sort(ids[clear], axis=1), np.sort(ti.numpy(), axis=1)), f"{name}: top-k set"
            want = np.zeros((int(clear.sum()), E), dtype=np.uint16)
            np.put_along_axis(want, ti.numpy(), bits_from_t(tw), axis=1)
            ulp = o.bf16_ulp_distance(w_bits[clear], np.take_along_axis(want, ids[clear].astype(np.int64), axis=1))
            assert ulp.max() <= 1, f"{name}: torch's CPU chain is {ulp.max()} bf16 ulps from the oracle"


def test_f64_to_bf16_gives_zero_for_zero():
    x = np.array([0.0, 1.0, 0.0, 2.0 ** -126, 1.8e-35])
    assert np.array_equal(mo.f64_to_bf16(x), np.array([0x0000, 0x3F80, 0x0000, 0x0080, 0x05BF], dtype=np.uint16))
