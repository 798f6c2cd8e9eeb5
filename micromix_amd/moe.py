"""`SparseMoEBlock`: the reference's `QMixtralSparseMoeBlock.forward` (model/qMixtralLayer.py:414-452) without its per-expert host loop.

The reference walks the experts in Python: `torch.where` on a one-hot mask, an index copy, the expert MLP (two quantizer launches and
three GEMMs, two `torch.cuda.synchronize()`), a scale by the routing weight and an `index_add_` -- about a hundred small launches
and over a dozen host syncs per layer.  Here the routing, the dispatch plan, the row gather and the combine are four device launches
(`mixedgemm.moe_route / moe_plan / moe_gather / moe_combine`) around the grouped quantizer and the grouped GEMM, which take every
expert's rows in one call.  The numbers are the reference's: the same expert rows through the same quantizer and GEMM, `F.silu(a) * b`
in torch bf16, and the combine adds a token's experts in ascending expert id with the reference's bf16 roundings.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from . import mixedgemm

__all__ = ["SparseMoEBlock"]

_PACKED = ("BN", "BS", "BO", "SFBN", "SFBS", "SFBO")


def _triple(expert):
    """(w1, w3, w2) of an expert given as an object with those attributes (QMixtralBlockSparseTop2MLP) or as a 3-sequence"""
    if all(hasattr(expert, n) for n in ("w1", "w3", "w2")):
        return expert.w1, expert.w3, expert.w2
    w1, w3, w2 = expert
    return w1, w3, w2


class SparseMoEBlock(nn.Module):
    """gate_weight: bf16 [E, H] (or a module with `.weight` / `.bias`, an nn.Linear); `gate_bias` optional bf16 [E].
    experts: E entries, each a `QLinearLayer` triple -- an object with `.w1`, `.w3`, `.w2` as QMixtralBlockSparseTop2MLP has them, or a
    (w1, w3, w2) sequence.  A layer carries its packed weights, its reorder index and its (p4, p6, p8) split; w1 and w3 read the same
    quantized rows, so they share index and split (the reference quantizes once, with w1's, qMixtralLayer.py:507-510), and all experts
    share the splits and the weight mode (their reorder indices are their own).  1 <= top_k <= 8, top_k <= E <= 64.

    `forward(hidden [.., H])` returns `(out [.., H], router_logits [T, E])` like the reference.  With the default `capturable=False` it
    reads the E + 1 expert offsets back to the host once, because the grouped entries take host row counts: that copy is the block's
    single sync, and in this mode the block is NOT hipGraph-capturable.  With `capturable=True` the expert quantizer and the expert GEMM
    read the row counts from the offsets on the device (`mixedgemm.moe_quantize / moe_matmul`): about ten launches whatever
    E is, no copy to the host, no per-expert Python loop, no allocation whose size depends on device data -- `forward` can be captured
    once per token count T and replayed on any routing.  The arithmetic is the default mode's, expert by expert, on the same kernel
    family; the bits are the default mode's wherever both modes split K over the same number of waves, and always when K <= 512 --
    with a longer K an expert of at most 64 rows may differ in the order of its fp32 partial sums, because the default mode picks the
    streaming configuration from the rows of each call and this mode from T ("Which bits").

    `fused_activation=True` (only with `capturable=True`, else ValueError) replaces the two torch launches of `F.silu(a) * b` and the
    quantizer behind them by one launch, `mixedgemm.moe_activate_quantize`, wherever the block takes the device-sized path (where it
    falls back to the host-sized path, the activation is torch's as before).  Which bits that gives: routing, plan, both
    up-projections, the down-projection GEMM and the combine are the capturable block's, unchanged; `h` is the device formula's,
    bf16(bf16(x * rcp(1 + exp2(-x log2 e))) * b), which equals torch's `F.silu(a) * b` except where the device `exp2` / `rcp` moves a
    value across a bf16 rounding boundary (fewer than 1 element in 1 000, none by more than 3 bf16 ulps).

    `fused_gate_up` (only with `capturable=True`, else ValueError; default False) replaces both up-projection GEMMs and the activation
    quantizer -- three launches -- by one, `mixedgemm.moe_gate_up_activate`: the tiled expert GEMM over the packed w1 | w3 weight with
    silu * mul and w2's quantizer in its epilogue.  `True` takes it at every T on the device-sized path; an int takes it from that many
    tokens on and the existing path below (below about 128 rows per expert the streaming kernels move the weight bytes faster than a
    128-row tile; the launch won from T = 128 on where it was measured, DESIGN.md 7e, and nothing is measured below, so the integer has no
    default).  It needs fp4 weights, no bias on w1 / w3 and a w2 split in 128s
    (ValueError at construction otherwise), and it keeps a second, row-permuted copy of w1 and w3: their memory doubles.  The bits are
    `fused_activation`'s for every expert of more than 64 rows; a smaller expert runs on the tiled kernels here and on the streaming
    kernels there, which may add the fp32 partial sums in another order.
    """

    def __init__(self, gate_weight, experts, top_k, gate_bias=None, capturable=False, fused_activation=False, fused_gate_up=False):
        super().__init__()
        if isinstance(gate_weight, nn.Module):
            gate_weight, gate_bias = gate_weight.weight, (gate_weight.bias if gate_bias is None else gate_bias)
        triples = [_triple(e) for e in experts]
        if not triples:
            raise ValueError("a sparse MoE block needs at least one expert")
        dev = triples[0][0].BN.device
        self.register_buffer("gate_weight", gate_weight.detach().to(device=dev, dtype=torch.bfloat16).contiguous())
        if gate_bias is not None:
            self.register_buffer("gate_bias", gate_bias.detach().to(device=dev, dtype=torch.bfloat16).contiguous())
        else:
            self.gate_bias = None
        self.num_experts, self.top_k = len(triples), int(top_k)
        if self.gate_weight.dim() != 2 or self.gate_weight.size(0) != self.num_experts:
            raise ValueError(f"gate_weight must be [E = {self.num_experts}, H]")
        if not (1 <= self.top_k <= 8 and self.top_k <= self.num_experts <= 64):
            raise ValueError("1 <= top_k <= 8 and top_k <= E <= 64")
        w1, w3, w2 = triples[0]
        self.hidden_dim, self.ffn_dim = w1.in_features, w1.out_features
        if self.gate_weight.size(1) != self.hidden_dim or self.hidden_dim % 8:
            raise ValueError("gate_weight must be [E, H] with H the experts' input width, a multiple of 8")
        self.split1 = (w1.p4_num, w1.p6_num, w1.p8_num)
        self.split2 = (w2.p4_num, w2.p6_num, w2.p8_num)
        self.rounding = w1.rounding
        for e, (a, b, c) in enumerate(triples):
            if (a.in_features, a.out_features, b.in_features, b.out_features, c.in_features, c.out_features) != \
                    (self.hidden_dim, self.ffn_dim, self.hidden_dim, self.ffn_dim, self.ffn_dim, self.hidden_dim):
                raise ValueError(f"expert {e}: w1 / w3 must be [I, H] and w2 [H, I] like expert 0's")
            if (a.p4_num, a.p6_num, a.p8_num) != self.split1 or (b.p4_num, b.p6_num, b.p8_num) != self.split1 or \
                    (c.p4_num, c.p6_num, c.p8_num) != self.split2:
                raise ValueError(f"expert {e}: the splits differ from expert 0's (or w3's from w1's)")
            if not torch.equal(a.reorder_index, b.reorder_index):
                raise ValueError(f"expert {e}: w1 and w3 read the same quantized rows and must share one reorder index")
            if any(l.rounding != self.rounding for l in (a, b, c)):
                raise ValueError(f"expert {e}: all layers must use one rounding mode")
        # references to the layers' own tensors (plain attributes of QLinearLayer), gathered once: one list per grouped call
        self._idx1 = [t[0].reorder_index for t in triples]
        self._idx2 = [t[2].reorder_index for t in triples]
        self._B = [[tuple(getattr(layer, n) for n in _PACKED) for layer in col] for col in zip(*triples)]     # w1s, w3s, w2s
        self._bias = [[layer.bias for layer in col] if any(layer.bias is not None for layer in col) else None for col in zip(*triples)]
        self.capturable = bool(capturable)
        self.fused_activation = bool(fused_activation)
        if self.fused_activation and not self.capturable:
            raise ValueError("fused_activation=True needs capturable=True: the fused activation exists for the device-sized launches only")
        # the token count from which forward takes the one-launch w1 | w3 path: None = never
        self._gate_up_from = None if fused_gate_up is False else (1 if fused_gate_up is True else int(fused_gate_up))
        if self._gate_up_from is not None and not self.capturable:
            raise ValueError("fused_gate_up needs capturable=True: the fused expert launch exists for the device-sized launches only")
        if self._gate_up_from is not None and self._gate_up_from < 1:
            raise ValueError("fused_gate_up must be True, False or a token count >= 1")
        self._supported = {}
        if self._gate_up_from is not None:      # the packed w1 | w3 table: a second copy of both weights, rows in w2's reordered order
            self._gate_up_table = mixedgemm.moe_gate_up_table(self._idx1, self._B[0], self._B[1], self._idx2, self.split1, self.split2,
                                                              biases1=self._bias[0], biases3=self._bias[1])
        if self.capturable:      # the device tables of the three layers (mm_moe_expert[E]), built once; they keep their tensors alive
            self._tables = [mixedgemm.moe_expert_table(idx, B, *split, biases=bias) for idx, B, split, bias in
                            zip((self._idx1, self._idx1, self._idx2), self._B, (self.split1, self.split1, self.split2), self._bias)]

    def _device_sized(self, T):
        """whether the expert GEMMs take device row counts at this T (asked once per T: very long K does not fit the streaming kernels'
        LDS, and the block then takes the host-sized path, which a capture cannot contain)"""
        ok = self._supported.get(T)
        if ok is None:
            ok = self._supported[T] = all(mixedgemm.moe_matmul_supported(T, t) for t in self._tables)
        if not ok and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"SparseMoEBlock(capturable=True): moe_matmul does not support these experts at T = {T} (K too long for the "
                               "weight-streaming kernels); the block would read the expert offsets on the host, which cannot be captured")
        return ok

    @torch.no_grad()
    def forward(self, hidden):
        shape, H, E = hidden.shape, self.hidden_dim, self.num_experts
        if hidden.dim() < 1 or hidden.size(-1) != H:          # (a width that H divides would otherwise reshape into other tokens)
            raise ValueError(f"hidden must be [.., H = {H}], got {tuple(shape)}")
        x = hidden.reshape(-1, H).contiguous()
        router_logits = F.linear(x, self.gate_weight, self.gate_bias)
        T = x.size(0)
        if T == 0:
            return hidden.new_zeros(shape), router_logits
        ids, w = mixedgemm.moe_route(router_logits, self.top_k)
        offsets, sorted_token, slot_of = mixedgemm.moe_plan(ids, E)
        if self.capturable and self._device_sized(T):
            # row counts stay on the device; a token meets an expert at most once, so no expert has more than T rows
            t1, t3, t2 = self._tables
            q1 = mixedgemm.moe_quantize(x, sorted_token, offsets, t1)          # the row gather is the quantizer's
            if self._gate_up_from is not None and T >= self._gate_up_from:
                q2 = mixedgemm.moe_gate_up_activate(q1, offsets, self._gate_up_table, T, self.split2, rounding=self.rounding)
                y = mixedgemm.moe_matmul(q2, offsets, t2, T, rounding=self.rounding)
                return mixedgemm.moe_combine(y, ids, w, slot_of).reshape(shape), router_logits
            a = mixedgemm.moe_matmul(q1, offsets, t1, T, rounding=self.rounding)
            b = mixedgemm.moe_matmul(q1, offsets, t3, T, rounding=self.rounding)
            if self.fused_activation:
                q2 = mixedgemm.moe_activate_quantize(a, b, offsets, t2)
            else:
                h = F.silu(a) * b
                q2 = mixedgemm.moe_quantize(h, None, offsets, t2)
            y = mixedgemm.moe_matmul(q2, offsets, t2, T, rounding=self.rounding)
            return mixedgemm.moe_combine(y, ids, w, slot_of).reshape(shape), router_logits
        xs = mixedgemm.moe_gather(x, sorted_token)
        off = offsets.tolist()                                # the block's single sync: the grouped entries take host row counts
        rows = lambda t: [t[off[e]:off[e + 1]] for e in range(E)]     # an expert without tokens is a group with M = 0
        n = T * self.top_k
        q1 = mixedgemm.reorder_quantize_x_grouped(rows(xs), self._idx1, *self.split1)
        a = torch.empty((n, self.ffn_dim), dtype=torch.bfloat16, device=x.device)
        b = torch.empty_like(a)
        mixedgemm.matmul_grouped(q1, self._B[0], biases=self._bias[0], rounding=self.rounding, outs=rows(a))
        mixedgemm.matmul_grouped(q1, self._B[1], biases=self._bias[1], rounding=self.rounding, outs=rows(b))
        h = F.silu(a) * b                                     # torch bf16, as the reference has it (act_fn(w1(x)) * w3(x))
        q2 = mixedgemm.reorder_quantize_x_grouped(rows(h), self._idx2, *self.split2)
        y = torch.empty((n, H), dtype=torch.bfloat16, device=x.device)
        mixedgemm.matmul_grouped(q2, self._B[2], biases=self._bias[2], rounding=self.rounding, outs=rows(y))
        out = mixedgemm.moe_combine(y, ids, w, slot_of)
        return out.reshape(shape), router_logits
