"""The sparse MoE block's ops, as `mixedgemm` exports them (include/micromix_hip.h, mm_moe_*): top-k routing, the dispatch plan, gather
and combine; the expert tables; and the device-sized grouped launches -- the expert quantizers, the expert GEMM and the fused
w1 | w3 -> silu * mul -> w2-quantizer launch -- whose row counts are read on the device.  micromix_amd/moe.py assembles the block.
None of it is an export of the reference module.  Every wrapper runs on torch's current stream and is capture-safe."""
from __future__ import annotations

import torch

from . import _lib
from ._args import _check_split, _check_tensor, _launch, _lead, _ok, _opt, _out, _ptr, _round_flags, _sf_bytes_w, _stream_ptr, _tensor

__all__ = ["moe_route", "moe_plan", "moe_gather", "moe_combine", "MoEExpertTable", "moe_expert_table", "moe_sf_bytes", "moe_quantize",
           "moe_activate_quantize", "moe_matmul", "moe_matmul_supported", "permute_packed_rows", "moe_gate_up_table", "moe_gate_up_activate",
           "moe_gate_up_activate_supported", "moe_gate_up_activate_describe"]


def moe_route(logits, top_k, *, topk_ids=None, topk_w=None):
    """Top-k routing of the gate logits: logits bf16 [T, E] -> (topk_ids int32 [T, top_k], topk_w bf16 [T, top_k]).

    Not an export of the reference module; the same numbers as its softmax(float) -> topk -> renormalise -> cast
    (qMixtralLayer.py:422-426): the top_k largest logits in descending order, equal logits in ascending expert index (torch.topk
    leaves ties unspecified), w_j = exp(l_j - max) / sum over the selected, in fp32, rounded to bf16.  1 <= top_k <= 8,
    top_k <= E <= 64.  Outputs are allocated unless passed in.  Runs on the current stream, capture-safe.
    """
    lib = _lib.load()
    dev = _lead(logits, "logits", torch.bfloat16)
    if logits.dim() != 2:
        raise RuntimeError("logits must be [T, E] bf16")
    (T, E), top_k = logits.shape, int(top_k)
    topk_ids = _out(topk_ids, "topk_ids", torch.int32, dev, (T, top_k))
    topk_w = _out(topk_w, "topk_w", torch.bfloat16, dev, (T, top_k))
    _launch("moe_route", dev, lib.mm_moe_route, _ptr(logits), T, E, top_k, _ptr(topk_ids), _ptr(topk_w), _stream_ptr(dev))
    return topk_ids, topk_w


def moe_plan(topk_ids, num_experts, *, expert_offsets=None, sorted_token=None, slot_of=None):
    """The dispatch plan of routed tokens: topk_ids int32 [T, top_k] -> (expert_offsets int32 [E + 1], sorted_token int32 [T * top_k],
    slot_of int32 [T, top_k]), a stable counting sort of the (token, k-slot) pairs by expert.

    Expert e owns the slots [expert_offsets[e], expert_offsets[e + 1]); within an expert the slots run by ascending token;
    sorted_token[s] is the token of slot s, slot_of[t, j] the slot of token t's j-th choice.  An id outside [0, E) is not counted and
    gets slot_of = -1; the slots left over then hold sorted_token = -1.  Deterministic; runs on the current stream, capture-safe.
    """
    lib = _lib.load()
    dev = _lead(topk_ids, "topk_ids", torch.int32)
    if topk_ids.dim() != 2:
        raise RuntimeError("topk_ids must be [T, top_k] int32")
    (T, top_k), E = topk_ids.shape, int(num_experts)
    i32 = torch.int32
    if expert_offsets is None:      # without tokens the entry does no device work: the offsets are all zero then
        expert_offsets = (torch.empty if T else torch.zeros)((max(E, 0) + 1,), dtype=i32, device=dev)
    else:
        _tensor(expert_offsets, "expert_offsets", i32, dev, (E + 1,))
        if T == 0:
            expert_offsets.zero_()
    sorted_token = _out(sorted_token, "sorted_token", i32, dev, (T * top_k,))
    slot_of = _out(slot_of, "slot_of", i32, dev, (T, top_k))
    _launch("moe_plan", dev, lib.mm_moe_plan, _ptr(topk_ids), T, E, top_k, _ptr(expert_offsets), _ptr(sorted_token), _ptr(slot_of), _stream_ptr(dev))
    return expert_offsets, sorted_token, slot_of


def moe_gather(x, sorted_token, *, out=None):
    """x bf16 [T, H], sorted_token int32 [n_rows] -> x_sorted bf16 [n_rows, H] with x_sorted[s] = x[sorted_token[s]] (H a multiple
    of 8).  A row whose sorted_token lies outside [0, T) is left as it was (uninitialised in an output allocated here).  Runs on the
    current stream, capture-safe."""
    lib = _lib.load()
    dev = _lead(x, "x", torch.bfloat16)
    if x.dim() != 2:
        raise RuntimeError("x must be [T, H] bf16")
    T, H = x.shape
    n_rows = _tensor(sorted_token, "sorted_token", torch.int32, dev).numel()
    out = _out(out, "out", torch.bfloat16, dev, (n_rows, H))
    _launch("moe_gather", dev, lib.mm_moe_gather, _ptr(x), _ptr(sorted_token), T, n_rows, H, _ptr(out), _stream_ptr(dev))
    return out


def moe_combine(y_sorted, topk_ids, topk_w, slot_of, *, out=None):
    """The weighted sum of every token's expert outputs: y_sorted bf16 [T * top_k, H] (rows in plan order), topk_ids int32, topk_w bf16,
    slot_of int32, all [T, top_k] -> out bf16 [T, H].

    Per token its entries are taken in ascending expert id, c = bf16(y * w), acc = bf16(acc + c) from +0.0: bit for bit what the
    reference's zeros + index_add_ expert by expert leaves (qMixtralLayer.py:428-450), whatever order topk_ids lists the experts in.
    Entries with slot_of = -1 are skipped; every row of out is written.  Runs on the current stream, capture-safe.
    """
    lib = _lib.load()
    dev = _lead(y_sorted, "y_sorted", torch.bfloat16)
    _tensor(topk_ids, "topk_ids", torch.int32, dev)
    if topk_ids.dim() != 2 or y_sorted.dim() != 2 or y_sorted.size(0) != topk_ids.numel():
        raise RuntimeError("topk_ids must be [T, top_k] and y_sorted [T * top_k, H]")
    T, top_k = topk_ids.shape
    H = y_sorted.size(1)
    _tensor(topk_w, "topk_w", torch.bfloat16, dev, (T, top_k))
    _tensor(slot_of, "slot_of", torch.int32, dev, (T, top_k))
    out = _out(out, "out", torch.bfloat16, dev, (T, H))
    _launch("moe_combine", dev, lib.mm_moe_combine, _ptr(y_sorted), _ptr(topk_ids), _ptr(topk_w), _ptr(slot_of), T, top_k, H, _ptr(out), _stream_ptr(dev))
    return out


# ---- device-sized grouped launches: the expert quantizer and GEMM of a capturable MoE block (mm_moe_quantize / mm_moe_matmul) ----

class MoEExpertTable:
    """`mm_moe_expert[E]` in device memory (include/micromix_hip.h) with the tensors it points to kept alive.  `tensor` int64 [E, 8]:
    per expert the addresses of (reorder_index, BN, BS, BO, SFBN, SFBS, SFBO, bias or 0).  Built once, by moe_expert_table."""
    __slots__ = ("tensor", "E", "N", "K", "split", "wmode", "has_bias", "_keep")


def moe_expert_table(reorder_indices, Bs, KN, KS, KO, biases=None):
    """One table per layer of the experts: reorder_indices[e] int16 [K], Bs[e] = (BN, BS, BO, SFBN, SFBS, SFBO) as matmul_grouped takes
    them, biases[e] bf16 [N] or None.  All experts share N, the (KN, KS, KO) split and the weight mode.  The addresses are copied to the
    device here -- build the table once (SparseMoEBlock.__init__), never per call."""
    E = len(Bs)
    if not (1 <= E <= 64) or len(reorder_indices) != E or (biases is not None and len(biases) != E):
        raise ValueError("1 <= E <= 64 experts, one reorder index (and bias entry) each")
    KN, KS, KO = int(KN), int(KS), int(KO)
    K = KN + KS + KO
    _check_split(KN, KS, KO, None, "moe_expert_table")
    dev = Bs[0][0].device
    index, u8 = dev.index, torch.uint8
    N = Bs[0][0].size(0)
    same = Bs[0][1].size(1) == KS // 4 * 3 and Bs[0][2].size(1) == KO          # (as matmul_grouped tells the weight mode)
    wmode = _lib.MM_W_MATCH if same else _lib.MM_W_FP4
    wb = (KN // 2, KS // 4 * 3 if same else KS // 2, KO if same else KO // 2)
    if tuple(tuple(t.shape) for t in Bs[0][:3]) != tuple((N, w) for w in wb):
        raise RuntimeError("the packed weights of expert 0 do not match the split in either weight mode")
    shapes = tuple(tuple(t.shape) for t in Bs[0])
    rows, keep = [], []
    for e, (idx, B) in enumerate(zip(reorder_indices, Bs)):
        if not _ok(idx, torch.int16, index) or idx.numel() != K:
            _check_tensor(idx, f"reorder_index[{e}]", torch.int16, dev)
            raise RuntimeError(f"expert {e}: the reorder index must have {K} entries")
        for t in B:
            if not _ok(t, u8, index):
                _check_tensor(t, f"expert {e} weight operand", u8, dev)
        if tuple(tuple(t.shape) for t in B[:3]) != shapes[:3] or any(t.numel() < _sf_bytes_w(N, k) for t, k in zip(B[3:], (KN, KS, KO))):
            raise RuntimeError(f"expert {e}: packed weights do not match N / split / weight mode of expert 0")
        bias = biases[e] if biases is not None else None
        if bias is not None and (not _ok(bias, torch.bfloat16, index) or bias.numel() != N):
            raise RuntimeError(f"expert {e}: bias must be a bfloat16 tensor with N elements")
        rows.append([idx.data_ptr()] + [t.data_ptr() if t.numel() else 0 for t in B] + [bias.data_ptr() if bias is not None else 0])
        keep.append((idx, B, bias))
    tab = MoEExpertTable()
    tab.tensor = torch.tensor(rows, dtype=torch.int64).to(dev)
    tab.E, tab.N, tab.K, tab.split, tab.wmode, tab._keep = E, N, K, (KN, KS, KO), wmode, keep
    tab.has_bias = biases is not None and any(b is not None for b in biases)
    return tab


def moe_sf_bytes(n, E, Kseg):
    """bytes of a packed scale tensor for n rows of E experts: n // 128 + E tiles of 128 rows (include/micromix_hip.h)"""
    return (n // 128 + E) * 128 * (Kseg // 32)


def _moe_outputs(out, n, E, widths, split, dev):
    """the 6-tuple a MoE quantizer fills: allocated, or the caller's `out` checked"""
    u8 = torch.uint8
    if out is None:
        return tuple(torch.empty((n, w), dtype=u8, device=dev) for w in widths) + \
            tuple(torch.empty((moe_sf_bytes(n, E, k),), dtype=u8, device=dev) for k in split)
    for t, w in zip(out[:3], widths):
        _tensor(t, "packed output", u8, dev, (n, w))
    for t, k in zip(out[3:], split):
        if _tensor(t, "scale output", u8, dev).numel() < moe_sf_bytes(n, E, k):
            raise RuntimeError("a scale output is smaller than moe_sf_bytes(n, E, Kseg)")
    return out


def _moe_operands(A, expert_offsets, table):
    """(device, n) of A = moe_quantize's 6-tuple (mode "x") of n rows in `table`'s split and of the plan's expert_offsets, checked"""
    dev = A[0].device
    E, (KN, KS, KO) = table.E, table.split
    n = A[0].size(0)
    u8 = torch.uint8
    for t, w in zip(A[:3], (KN // 2, KS // 4 * 3, KO)):
        _tensor(t, "activation segment", u8, dev, (n, w))
    for t, k in zip(A[3:], (KN, KS, KO)):
        if _tensor(t, "activation scales", u8, dev).numel() < moe_sf_bytes(n, E, k):
            raise RuntimeError("an activation scale tensor is smaller than moe_sf_bytes(n, E, Kseg)")
    _tensor(expert_offsets, "expert_offsets", torch.int32, dev, (E + 1,))
    return dev, n


def moe_quantize(src, row_of_slot, expert_offsets, table, n=None, *, mode="x", out=None):
    """The expert quantizer with the row counts read on the device: for every slot s that an expert owns (expert_offsets int32 [E + 1],
    moe_plan's), row row_of_slot[s] of src bf16 [rows, K] -- row s itself with row_of_slot=None -- quantized with that expert's reorder
    index (table: moe_expert_table).  Returns ONE 6-tuple (oN, oS, oO, sfN, sfS, sfO) for all experts: packed rows in slot order
    [n, .], scale tensors of moe_sf_bytes(n, E, Kseg) bytes with expert e's run at tile expert_offsets[e] // 128 + e; bytes of slots and
    tiles that no expert owns are left as they were.  n defaults to len(row_of_slot) (or src's rows).  mode "x" (mixed) or "w4".
    Byte for byte reorder_quantize_x_grouped's per-expert tensors laid end to end.  No host sync; capture-safe."""
    lib = _lib.load()
    dev = _lead(src, "src", torch.bfloat16)
    if src.dim() != 2:
        raise RuntimeError("src must be [rows, K] bf16")
    src_rows, K = src.shape
    if mode not in ("x", "w4"):
        raise ValueError("mode must be 'x' or 'w4'")
    w4 = mode == "w4"
    E, (KN, KS, KO) = table.E, table.split
    if K != table.K:
        raise RuntimeError(f"src must be [rows, {table.K}]")
    _tensor(expert_offsets, "expert_offsets", torch.int32, dev, (E + 1,))
    if row_of_slot is not None:
        _tensor(row_of_slot, "row_of_slot", torch.int32, dev)
        n = row_of_slot.numel() if n is None else int(n)
        if row_of_slot.numel() < n:
            raise RuntimeError("row_of_slot must have n entries")
    else:
        n = src_rows if n is None else int(n)
    out = _moe_outputs(out, n, E, (KN // 2, KS // 2 if w4 else KS // 4 * 3, KO // 2 if w4 else KO), (KN, KS, KO), dev)
    _launch("moe_quantize", dev, lib.mm_moe_quantize, _ptr(src), _opt(row_of_slot), _ptr(expert_offsets), _ptr(table.tensor), E, n, src_rows, K,
            KN, KS, KO, _lib.MM_QUANT_W4 if w4 else _lib.MM_QUANT_MIXED, *(_ptr(t) for t in out), _stream_ptr(dev))
    return tuple(out)


def moe_activate_quantize(a, b, expert_offsets, table, *, out=None, h_out=None):
    """The experts' activation and the quantizer of their down-projection in one launch: a, b bf16 [n, K] in slot order (the outputs of
    moe_matmul for w1 and w3), and for every slot s that an expert owns h[s] = bf16(bf16(silu(a[s])) * b[s]) -- torch's bf16
    `F.silu(a) * b` except where the device exp2 / rcp move a value across a bf16 rounding boundary (include/micromix_hip.h) --
    quantized as moe_quantize(h, None, expert_offsets, table) would.  Returns that 6-tuple, byte for byte; `out=` takes a 6-tuple to
    fill.  h_out: None, or a bf16 [n, K] tensor (not a or b) that also receives h.  Slots no expert owns are left as they were in
    every output.  Mixed mode only.  No host sync, no allocation sized by device data; capture-safe."""
    lib = _lib.load()
    dev = _lead(a, "a", torch.bfloat16)
    if a.dim() != 2:
        raise RuntimeError("a must be [n, K] bf16")
    n, K = a.shape
    _tensor(b, "b", torch.bfloat16, dev, (n, K))
    E, (KN, KS, KO) = table.E, table.split
    if K != table.K:
        raise RuntimeError(f"a and b must be [n, {table.K}]")
    _tensor(expert_offsets, "expert_offsets", torch.int32, dev, (E + 1,))
    if h_out is not None:
        _tensor(h_out, "h_out", torch.bfloat16, dev, (n, K))
        if h_out.data_ptr() in (a.data_ptr(), b.data_ptr()) and n:
            raise RuntimeError("h_out must not be a or b")
    out = _moe_outputs(out, n, E, (KN // 2, KS // 4 * 3, KO), (KN, KS, KO), dev)
    _launch("moe_activate_quantize", dev, lib.mm_moe_activate_quantize, _ptr(a), _ptr(b), _ptr(expert_offsets), _ptr(table.tensor), E, n, K,
            KN, KS, KO, *(_ptr(t) for t in out), _opt(h_out), _stream_ptr(dev))
    return tuple(out)


def moe_matmul_supported(max_rows, table):
    """False where moe_matmul would answer "unsupported configuration" (very long K: take matmul_grouped there)"""
    return bool(_lib.load().mm_moe_matmul_supported(int(max_rows), table.N, *table.split, table.wmode))


def moe_matmul(A, expert_offsets, table, max_rows, *, rounding="reference", out=None):
    """The expert GEMM with the row counts read on the device: A = moe_quantize's 6-tuple (mode "x"), out bf16 [n, N] with the rows of
    expert e = matmul_grouped's output for that expert (bit for bit wherever both split K over the same number of waves, and always when
    K <= 512: include/micromix_hip.h), weights and biases from `table`.  max_rows: a bound on any expert's
    rows that the caller vouches for (T in a MoE block); an expert with more rows is skipped, its rows of `out` left as they were, as
    are the rows from expert_offsets[E] on.  At most two launches, whatever E.  No host sync; capture-safe."""
    lib = _lib.load()
    if rounding not in ("reference", "fused"):
        _round_flags(rounding)
    flags = _lib.MM_ROUND_PER_SEGMENT if rounding == "reference" else _lib.MM_ROUND_ONCE
    dev, n = _moe_operands(A, expert_offsets, table)
    out = _out(out, "out", torch.bfloat16, dev, (n, table.N))
    _launch("moe_matmul", dev, lib.mm_moe_matmul, *(_ptr(t) for t in A), _ptr(expert_offsets), _ptr(table.tensor), table.E, n, int(max_rows),
            table.N, *table.split, table.wmode, flags, _ptr(out), _stream_ptr(dev))
    return out


# ---- w1 | w3, silu * mul and w2's quantizer in one expert launch (mm_moe_gate_up_activate) ----

def permute_packed_rows(packed6, perm):
    """Rows of a packed weight (BN, BS, BO, SFBN, SFBS, SFBO) in another order: row j of the result is row perm[j] of the input.

    Weights are quantized per output row, so this is a pure byte shuffle, equal byte for byte to quantizing the row-permuted weight:
    the packed codes move as rows; a scale tensor is tiled per 128 rows, and inside a tile's 512-byte atom of one 128-column slab row
    r sits at (r & 31) * 16 + ((r >> 5) & 3) * 4 (sf_offset, csrc/mx_common.h).  The row count must be a multiple of 128 (whole scale
    tiles) and perm a permutation of it.  Plain torch on any device, CPU tensors included; returns new tensors."""
    n = packed6[0].size(0)
    perm = torch.as_tensor(perm).to(device=packed6[0].device, dtype=torch.long).reshape(-1)
    if n % 128 or perm.numel() != n or (n and not torch.equal(torch.sort(perm).values, torch.arange(n, device=perm.device))):
        raise ValueError("permute_packed_rows: the rows must be a multiple of 128 and perm a permutation of them")
    out = [t.index_select(0, perm) if t.numel() else t.clone() for t in packed6[:3]]
    for t in packed6[3:]:
        if t.numel() == 0:
            out.append(t.clone())
            continue
        if t.numel() % (n * 4):
            raise ValueError("permute_packed_rows: a scale tensor is not whole 128-row tiles of these rows")
        atoms = t.numel() // (n * 4)                                  # 128-column slabs of the segment
        rows = t.reshape(n // 128, atoms, 32, 4, 4).permute(0, 3, 2, 1, 4).reshape(n, atoms * 4)        # [row, its scale bytes]
        rows = rows.index_select(0, perm)
        out.append(rows.reshape(n // 128, 4, 32, atoms, 4).permute(0, 3, 2, 1, 4).reshape(-1).contiguous())
    return tuple(out)


def moe_gate_up_table(reorder_indices1, w1s, w3s, reorder_indices2, split1, split2, *, biases1=None, biases3=None):
    """The device table of `moe_gate_up_activate`: per expert ONE packed fp4 weight of N = 2 I rows made from w1s[e] and w3s[e] (the
    6-tuples moe_expert_table takes).  Row j of the gate half is w1 row reorder_indices2[e][j], row j of the up half is w3 row
    reorder_indices2[e][j] -- the expert's w2 reorder index moves into the weight, because the fused epilogue quantizes 128 consecutive
    features into one segment of w2's K split -- and the halves are interleaved per 128 rows (interleave_gate_up).  reorder_indices1[e]
    is the index of the first quantizer (w1's), split1 / split2 the (KN, KS, KO) splits of w1 and of w2.  Returns a MoEExpertTable with
    N = 2 I and no bias whose weights are NEW tensors that it keeps alive: while the originals stay in use elsewhere, the memory held
    for w1 / w3 doubles.  Raises ValueError for biases on w1 / w3, weights that are not fp4 (MM_W_FP4), I not a multiple of 128 or an
    entry of split2 that is not a multiple of 128 (or split2 not adding up to I)."""
    from .mixedgemm import interleave_gate_up       # (mixedgemm re-exports this module: not at import time)
    E = len(w1s)
    if not (1 <= E <= 64) or len(w3s) != E or len(reorder_indices1) != E or len(reorder_indices2) != E:
        raise ValueError("moe_gate_up_table: 1 <= E <= 64 experts with w1, w3 and both reorder indices each")
    if any(b is not None for bs in (biases1, biases3) if bs is not None for b in bs):
        raise ValueError("moe_gate_up_table: w1 / w3 must have no bias (the fused epilogue adds none)")
    KN, KS, KO = (int(k) for k in split1)
    split2 = tuple(int(k) for k in split2)
    I = w1s[0][0].size(0)
    if I < 128 or I % 128:
        raise ValueError(f"moe_gate_up_table: I = {I} must be a multiple of 128")
    if len(split2) != 3 or any(k < 0 or k % 128 for k in split2) or sum(split2) != I:
        raise ValueError(f"moe_gate_up_table: split2 = {split2} must be three non-negative multiples of 128 that add up to I = {I}")
    fp4 = ((I, KN // 2), (I, KS // 2), (I, KO // 2))
    Bs = []
    for e in range(E):
        for name, B in (("w1", w1s[e]), ("w3", w3s[e])):
            if tuple(tuple(t.shape) for t in B[:3]) != fp4:
                raise ValueError(f"moe_gate_up_table: expert {e}: {name} must be fp4 weights (MM_W_FP4) of [{I}, .] rows matching split1")
            if any(t.numel() < _sf_bytes_w(I, k) for t, k in zip(B[3:], (KN, KS, KO))):
                raise ValueError(f"moe_gate_up_table: expert {e}: a scale tensor of {name} holds fewer than _sf_bytes_w(I, Kseg) bytes")
        idx2 = reorder_indices2[e]
        if idx2.numel() != I:
            raise ValueError(f"moe_gate_up_table: expert {e}: w2's reorder index must have I = {I} entries")
        whole = lambda B: tuple(B[:3]) + tuple(t.reshape(-1)[:_sf_bytes_w(I, k)] for t, k in zip(B[3:], (KN, KS, KO)))
        Bs.append(interleave_gate_up(permute_packed_rows(whole(w1s[e]), idx2), permute_packed_rows(whole(w3s[e]), idx2)))
    tab = moe_expert_table(reorder_indices1, Bs, KN, KS, KO)
    tab.wmode = _lib.MM_W_FP4              # (moe_expert_table cannot tell the modes apart when KS = KO = 0)
    return tab


def _gate_up_split2(table, split2):
    DN, DS, DO = (int(k) for k in split2)
    if table.N % 256:
        raise RuntimeError("table must be a moe_gate_up_table (N = 2 I, I a multiple of 128)")
    _check_split(DN, DS, DO, table.N // 2, "moe_gate_up_activate")
    return DN, DS, DO


def moe_gate_up_activate_supported(max_rows, table, split2):
    """False where moe_gate_up_activate would refuse: max_rows < 1, a bad split, or a table whose weights are not fp4"""
    I = table.N // 2
    return table.N % 256 == 0 and bool(_lib.load().mm_moe_gate_up_activate_supported(int(max_rows), I, *table.split, *(int(k) for k in split2), table.wmode))


def moe_gate_up_activate_describe(table, n, split2=None):
    """which kernel family and how many workgroups moe_gate_up_activate launches for n rows on the current device"""
    return _lib.load().mm_moe_gate_up_activate_describe(table.E, int(n), table.N // 2).decode()


def moe_gate_up_activate(A, expert_offsets, table, max_rows, split2, *, rounding="reference", out=None):
    """Both up-projections of the experts, silu * mul and the quantizer of their down-projection in ONE launch: A = moe_quantize's
    6-tuple (mode "x", w1's split), table = moe_gate_up_table(..), split2 = w2's (KN, KS, KO).  Returns the 6-tuple that moe_matmul
    takes for w2 -- for every slot an expert of 1 .. max_rows rows owns byte for byte what
    `moe_activate_quantize(moe_matmul(A, .., w1), moe_matmul(A, .., w3), offsets, w2's table)` gives wherever moe_matmul runs the
    expert on the tiled kernels (more than 64 rows; below that it may add its fp32 partial sums in another order, include/micromix_hip.h).
    Scale bytes of rows past an expert's last inside its own 128-row tiles are unspecified; everything else outside the experts' rows
    and runs, and the rows of an expert above max_rows, are left as they were.  `out=` takes a 6-tuple to fill.  No host sync, no
    allocation sized by device data; capture-safe."""
    lib = _lib.load()
    if rounding not in ("reference", "fused"):
        _round_flags(rounding)
    flags = _lib.MM_ROUND_PER_SEGMENT if rounding == "reference" else _lib.MM_ROUND_ONCE
    DN, DS, DO = _gate_up_split2(table, split2)
    dev, n = _moe_operands(A, expert_offsets, table)
    out = _moe_outputs(out, n, table.E, (DN // 2, DS // 4 * 3, DO), (DN, DS, DO), dev)
    _launch("moe_gate_up_activate", dev, lib.mm_moe_gate_up_activate, *(_ptr(t) for t in A), _ptr(expert_offsets), _ptr(table.tensor), table.E, n,
            int(max_rows), table.N // 2, *table.split, DN, DS, DO, flags, *(_ptr(t) for t in out), _stream_ptr(dev))
    return tuple(out)
