"""GPU tests of micromix_amd.moe.SparseMoEBlock over the configurations it accepts (tests/moe_block_oracle.py: H != I, split1 != split2,
empty segments, both weight modes, both roundings, experts with and without biases, E up to 64) with the rows per expert scripted, in
three layers per case:

  a. the block bit-equal to the reference's per-expert loop (tests/test_moe_gpu.py's `reference_loop`, here with bias, rounding and
     weight mode), 2-D and 3-D input, two calls;
  b. every stage of that loop against the oracle on the GPU's own input to it: route, the quantized rows byte for byte, the three GEMMs
     per expert within tests/gemm_check.py (its statistics over the case: GemmPopulation), h within 2 bf16 ulps (torch's op: one ulp
     per rounding), the combine bit for bit;
  c. the block against the oracle block run on its own intermediates: d1 = |gpu - oracle| / |oracle| below d0 = |oracle - unquantized| /
     |unquantized|, the noise of the number formats themselves, measured in the same test.  A wrong expert's weights or a swapped
     split, used consistently by block and loop, pass (a) and (b) and give d1 of the order of 1.
"""
import numpy as np
import pytest

import moe_block_oracle as mb
import moe_oracle as mo
from conftest import bits_from_t, t_from_bits, u8
from gemm_check import FRAC_EXACT, FRAC_GT1, MAX_ULP, check_gemm
from micromix_amd import mixedgemm
from model_case import gen_bf16
from oracle import mx_oracle as o

pytestmark = pytest.mark.gpu
PACKED = ("BN", "BS", "BO", "SFBN", "SFBS", "SFBO")


class Built:
    """one configuration on the device: the drawn tensors, the QLinearLayer triples, and the same experts for the oracle"""

    def __init__(self, cfg_id, dev):
        import torch
        from micromix_amd.qlinear import QLinearLayer
        self.cfg = cfg = mb.CONFIGS[cfg_id]
        self.drawn = mb.draw_experts(cfg, dev, seed=1000 * (1 + "ABCDE".index(cfg_id)))
        self.oracle = mb.oracle_experts(cfg, self.drawn)
        self.anchored = set()

        def layer(w, bias, index, split):
            lin = torch.nn.Linear(w.size(1), w.size(0), bias=bias is not None, dtype=torch.bfloat16, device=dev)
            lin.weight.data = w
            if bias is not None:
                lin.bias.data = bias
            return QLinearLayer(lin, p8_num=split[2], p6_num=split[1], reorder_index=index, weight_mode=cfg["wmode"], rounding=cfg["rounding"])

        self.layers = [(layer(d["w"][0], d["bias"][0], d["idx1"], cfg["split1"]), layer(d["w"][1], d["bias"][1], d["idx1"], cfg["split1"]),
                        layer(d["w"][2], d["bias"][2], d["idx2"], cfg["split2"])) for d in self.drawn]


@pytest.fixture(scope="module")
def built(dev):
    """configuration id -> Built, made once per module (configuration C has 192 layers)"""
    cache = {}

    def get(cfg_id):
        if cfg_id not in cache:
            cache[cfg_id] = Built(cfg_id, dev)
        return cache[cfg_id]
    return get


def reference_loop(x, gate_w, gate_b, experts, top_k, stages):
    """`reference_loop` of tests/test_moe_gpu.py with every layer's own bias and rounding (and whatever weight mode it was packed in),
    keeping each expert's intermediates in `stages`"""
    import torch
    import torch.nn.functional as F
    mm = lambda q, l: mixedgemm.matmul(q[0], l.BN, q[1], l.BS, q[2], l.BO, q[3], l.SFBN, q[4], l.SFBS, q[5], l.SFBO, bias=l.bias,
                                       rounding=l.rounding, split_k=False)
    logits = F.linear(x, gate_w, gate_b)
    ids, w = mixedgemm.moe_route(logits, top_k)
    final = torch.zeros_like(x)
    mask = torch.nn.functional.one_hot(ids.long(), num_classes=len(experts)).permute(2, 1, 0)
    for e, (w1, w3, w2) in enumerate(experts):
        idx, top_x = torch.where(mask[e])
        if top_x.numel() == 0:
            continue
        cur = x[None, top_x].reshape(-1, x.size(1))
        q1 = mixedgemm.reorder_quantize_x(cur, w1.reorder_index, w1.p4_num, w1.p6_num, w1.p8_num)
        a, b = mm(q1, w1), mm(q1, w3)
        h = F.silu(a) * b
        q2 = mixedgemm.reorder_quantize_x(h, w2.reorder_index, w2.p4_num, w2.p6_num, w2.p8_num)
        y = mm(q2, w2)
        final.index_add_(0, top_x, y * w[top_x, idx, None])
        stages.append(dict(e=e, slot=idx, token=top_x, x=cur, q1=q1, a=a, b=b, h=h, q2=q2, y=y))
    return final, logits, ids, w


def assert_quantized(got, want, rows, split, label):
    for i in range(3):
        if split[i]:
            assert np.array_equal(u8(got[i]), want[i]), f"{label}: packed segment {i}"
            offs = o.sf_valid_offsets(rows, split[i])
            assert np.array_equal(u8(got[3 + i])[offs], want[3 + i][offs]), f"{label}: scales of segment {i}"


class GemmPopulation:
    """tests/gemm_check.py states a tolerance per output element and, with strict=True, three statistics measured over full model
    shapes: the share of outputs more than one ulp off, the share of bit-equal ones, the largest ulp distance away from cancellation.
    Every expert's product is held to the per-element tolerance, and to the last of the three, on its own; the two shares need a
    population -- one expert may have a single row -- so they are taken over all the products of a case, with that file's numbers and
    its own allowance for small populations (3 outputs; no bit-equal share below 4096 outputs)."""

    def __init__(self, wmode):
        self.wmode, self.n, self.gt1, self.exact = wmode, 0, 0.0, 0.0

    def check(self, got_bits, *args, label, **kw):
        st = check_gemm(got_bits, *args, label=label, **kw)
        assert st["max_ulp_noncancelling"] <= MAX_ULP, f"{label}: ulp statistics {st}"
        self.n, self.gt1, self.exact = self.n + got_bits.size, self.gt1 + st["frac_gt1"] * got_bits.size, self.exact + st["frac_exact"] * got_bits.size

    def assert_shares(self, label):
        gt1, exact = self.gt1 / self.n, self.exact / self.n
        print(f"{label}: {self.n} GEMM outputs, {100 * exact:.2f} % bit-equal to the oracle, {100 * gt1:.3f} % more than one ulp off")
        assert gt1 <= max(FRAC_GT1[self.wmode], 3.0 / self.n) and (exact >= FRAC_EXACT[self.wmode] or self.n < 4096), (label, gt1, exact)


def check_block(dev, B, gate_bits, x_bits, label, counts=None, forced_ids=None):
    import torch
    from micromix_amd import SparseMoEBlock
    cfg = B.cfg
    E, k, H, I = cfg["E"], cfg["k"], cfg["H"], cfg["I"]
    T = x_bits.shape[0]
    x, gate_w = t_from_bits(x_bits, dev), t_from_bits(gate_bits, dev)
    block = SparseMoEBlock(gate_w, B.layers, k)
    assert (block.hidden_dim, block.ffn_dim, block.split1, block.split2, block.rounding) == (H, I, cfg["split1"], cfg["split2"], cfg["rounding"])
    assert [[b is not None for b in col] if col is not None else None for col in block._bias] == \
        [[mb.bias_layers(cfg, e)[i] for e in range(E)] if any(mb.bias_layers(cfg, e)[i] for e in range(E)) else None for i in range(3)]

    # ---- a. the block against the per-expert loop, bit for bit -------------------------------------------------------------------
    out, logits = block(x)
    stages = []
    want, want_logits, ids, w = reference_loop(x, gate_w, None, B.layers, k, stages)
    lead = (2, T // 2) if T % 2 == 0 else (1, T)
    out3, logits3 = block(x.reshape(*lead, H))
    out2, logits2 = block(x)
    torch.cuda.synchronize()
    ids_h, w_bits, logit_bits = u8(ids), bits_from_t(w), bits_from_t(logits)
    got_counts = np.bincount(ids_h.reshape(-1), minlength=E)
    print(f"{label}: rows per expert {got_counts.tolist()}")
    if counts is not None:
        assert np.array_equal(got_counts, counts), "the routing is not the scripted one"
        assert np.array_equal(ids_h, forced_ids) and np.array_equal(logit_bits, mb.scripted_logit_bits(forced_ids, E))
    assert tuple(out.shape) == (T, H) and tuple(out3.shape) == (*lead, H) and tuple(logits.shape) == (T, E) and tuple(logits3.shape) == (T, E)
    assert torch.equal(logits, want_logits) and torch.equal(logits3, want_logits) and torch.equal(logits2, want_logits)
    assert bool(torch.isfinite(want).all()) and float(want.float().abs().max()) > 0
    assert torch.equal(out, want), "the block differs from the per-expert loop"
    assert torch.equal(out3.reshape(T, H), want) and torch.equal(out2, want)

    # ---- b. every stage of the loop against the oracle on the GPU's own input to it -----------------------------------------------
    want_ids, want_w, _ = mo.route(logit_bits, k)
    assert np.array_equal(ids_h, want_ids) and o.bf16_ulp_distance(w_bits, want_w).max() <= 1
    offsets, _, slot_of = mo.plan(ids_h, E)
    assert [s["e"] for s in stages] == np.flatnonzero(got_counts).tolist()
    y_sorted = np.zeros((T * k, H), dtype=np.uint16)
    worst_h, gemms = 0, GemmPopulation(cfg["wmode"])
    for s in stages:
        e, ex, rows = s["e"], B.oracle[s["e"]], s["x"].size(0)
        assert rows == got_counts[e]
        if e not in B.anchored:                               # the packed weights the GEMMs read are the oracle's, byte for byte
            for i, layer in enumerate(B.layers[e]):
                assert_quantized([getattr(layer, n) for n in PACKED], ex.packed(i), layer.out_features, ex.split[i], f"{label} expert {e} weight {i}")
            B.anchored.add(e)
        assert np.array_equal(bits_from_t(s["x"]), x_bits[u8(s["token"])])
        q1 = ex.quantize(bits_from_t(s["x"]), 0)
        assert_quantized(s["q1"], q1, rows, cfg["split1"], f"{label} expert {e} x")
        for i, name in ((0, "a"), (1, "b")):
            gemms.check(bits_from_t(s[name]), q1, ex.packed(i), cfg["rounding"], label=f"{label} expert {e} w{(1, 3)[i]} M={rows}",
                        wdeq=ex.deq(i), bias_bits=ex.bias_bits[i])
        ulp = o.bf16_ulp_distance(bits_from_t(s["h"]), mb.silu_mul_bf16(bits_from_t(s["a"]), bits_from_t(s["b"])))
        worst_h = max(worst_h, int(ulp.max()))
        assert ulp.max() <= 2, f"{label} expert {e}: silu(a) * b is {ulp.max()} bf16 ulps from the two-rounding fp64 expression"
        q2 = ex.quantize(bits_from_t(s["h"]), 2)
        assert_quantized(s["q2"], q2, rows, cfg["split2"], f"{label} expert {e} h")
        gemms.check(bits_from_t(s["y"]), q2, ex.packed(2), cfg["rounding"], label=f"{label} expert {e} w2 M={rows}",
                    wdeq=ex.deq(2), bias_bits=ex.bias_bits[2])
        y_sorted[slot_of[u8(s["token"]), u8(s["slot"])]] = bits_from_t(s["y"])
    gemms.assert_shares(label)
    assert np.array_equal(mo.combine(y_sorted, ids_h, w_bits, slot_of), bits_from_t(want)), "combine"

    # ---- c. the block against the oracle block on its own intermediates ---------------------------------------------------------
    chain = mb.oracle_block(x_bits, B.oracle, k, logit_bits)
    plain = mb.unquantized_block(x_bits, B.oracle, chain["ids"], chain["w"])
    d1 = mb.relative_distance(o.bf16_to_f32(bits_from_t(out)), o.bf16_to_f32(chain["out"]))
    d0 = mb.relative_distance(o.bf16_to_f32(chain["out"]), plain)
    print(f"parity {label}: d1 = |gpu - oracle| / |oracle| = {d1:.5f}, d0 = |oracle - unquantized| / |unquantized| = {d0:.5f}, "
          f"h at most {worst_h} ulp from the oracle's")
    assert d1 < d0, (d1, d0)
    return got_counts


@pytest.mark.parametrize("name", list(mb.SCRIPTED))
def test_block_with_scripted_routing(dev, built, name):
    cfg_id, T, counts = mb.SCRIPTED[name]
    B = built(cfg_id)
    cfg = B.cfg
    base = bits_from_t(gen_bf16(dev, T, cfg["H"], 900 + T, "x"))
    x_bits, ids = mb.scripted_x(counts, T, cfg["k"], base)
    check_block(dev, B, mb.gate_unit_bits(cfg["E"], cfg["H"]), x_bits, name, counts=np.asarray(counts), forced_ids=ids)


def test_block_c_with_a_gaussian_gate(dev, built):
    """E = 64, k = 8, T = 40: 320 rows wherever the gate puts them -- nothing scripted, so only what bincount shows is asserted: experts
    with and without rows, and more non-empty ones than one grouped launch takes"""
    B = built("C")
    cfg = B.cfg
    T = 40
    gate = o.f32_to_bf16((0.05 * np.random.default_rng(64).standard_normal((cfg["E"], cfg["H"]))).astype(np.float32))
    counts = check_block(dev, B, gate, bits_from_t(gen_bf16(dev, T, cfg["H"], 940, "x")), "C gaussian gate T=40")
    assert counts.sum() == T * cfg["k"] and counts.max() <= T and (counts > 0).sum() > 8


def test_block_rejects_mismatched_layers_and_inputs(dev, built):
    import torch
    from micromix_amd import SparseMoEBlock
    from micromix_amd.qlinear import QLinearLayer
    B = built("A")
    cfg = B.cfg
    E, k, H, I = cfg["E"], cfg["k"], cfg["H"], cfg["I"]
    gate = t_from_bits(mb.gate_unit_bits(E, H), dev)

    def layer(w, index, split):
        lin = torch.nn.Linear(w.size(1), w.size(0), bias=False, dtype=torch.bfloat16, device=dev)
        lin.weight.data = w
        return QLinearLayer(lin, p8_num=split[2], p6_num=split[1], reorder_index=index)

    # w2 layers with split1's widths: layers over H, as w1 is, where [H, I] layers over split2 belong
    over_h = [(a, b, layer(d["w"][2][:, :H].contiguous(), d["idx1"], cfg["split1"])) for (a, b, c), d in zip(B.layers, B.drawn)]
    assert all((c.p4_num, c.p6_num, c.p8_num) == cfg["split1"] for _, _, c in over_h)
    with pytest.raises(ValueError):
        SparseMoEBlock(gate, over_h, k)
    # one expert whose w2 has another split than expert 0's
    d = B.drawn[3]
    other = list(B.layers)
    other[3] = (other[3][0], other[3][1], layer(d["w"][2], d["idx2"], (128, 256, 128)))
    with pytest.raises(ValueError):
        SparseMoEBlock(gate, other, k)
    # ... and one whose w1 / w3 have
    other = list(B.layers)
    other[5] = (layer(B.drawn[5]["w"][0], B.drawn[5]["idx1"], (0, 128, 128)), layer(B.drawn[5]["w"][1], B.drawn[5]["idx1"], (0, 128, 128)), other[5][2])
    with pytest.raises(ValueError):
        SparseMoEBlock(gate, other, k)
    # a last dimension that is not H -- 2 H and H / 2 would reshape into other tokens, I is w2's width
    block = SparseMoEBlock(gate, B.layers, k)
    for width in (2 * H, H // 2, I, H + 8):
        with pytest.raises(ValueError):
            block(torch.zeros((4, width), dtype=torch.bfloat16, device=dev))
        with pytest.raises(ValueError):
            block(torch.zeros((2, 2, width), dtype=torch.bfloat16, device=dev))
    out, logits = block(torch.zeros((2, 2, H), dtype=torch.bfloat16, device=dev))
    assert tuple(out.shape) == (2, 2, H) and tuple(logits.shape) == (4, E)
