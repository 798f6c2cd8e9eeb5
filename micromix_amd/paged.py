"""The paged KV cache and what runs over it, as `mixedgemm` exports it: append (with RoPE), page copy and row moves, decode, shared-prefix
decode and prefill attention (include/micromix_hip.h, mm_kv_append .. mm_paged_prefill_tree), the end of a speculative step:
`process_logits` (include/micromix_logits.h) -> `argmax_rows` / `sample_rows` / `spec_sample_rows` (include/micromix_spec.h; `uniform_rows`,
include/micromix_random.h, makes their uniform numbers from the request's seed and the position) ->
`verify_greedy` -> `token_step` (include/micromix_tokens.h: the token history's half of a step; `ngram_draft` drafts the next chain from
it) -> `kv_step` (include/micromix_kvstep.h: the page table's bookkeeping between two steps), and what the logits say about a
token: `logprob_rows` / `cross_entropy` (include/micromix_logprob.h).  None of it is an export of the reference module (its append_kv_i4 / _f16 take K/V
already quantized and one head count); micromix_amd/kvcache.py is the small cache object on top.  Every wrapper runs on torch's
current stream and is capture-safe."""
from __future__ import annotations

from collections import namedtuple

import torch

from . import _lib
from ._args import _check_tensor, _launch, _lead, _lib_with, _ok, _opt, _out, _ptr, _stream_ptr, _tensor

__all__ = ["kv_append", "rope_kv_append", "kv_copy_pages", "kv_move_rows", "kv_step", "kv_step_state_ints", "paged_decode", "paged_decode_workspace_bytes", "paged_decode_shared",
           "paged_decode_shared_workspace_bytes", "paged_prefill", "paged_prefill_workspace_bytes", "argmax_rows", "argmax_rows_workspace_bytes",
           "verify_greedy", "sample_rows", "sample_rows_workspace_bytes", "logprob_rows", "logprob_rows_workspace_bytes", "cross_entropy",
           "process_logits", "spec_sample_rows", "spec_sample_rows_workspace_bytes", "chain_candidates", "token_step", "ngram_draft",
           "ngram_draft_workspace_bytes", "uniform_rows"]

# entries a library built before them lacks: (the symbol looked for, the names and the feature of the rebuild message)
_TREE = ("mm_paged_prefill_tree", "mm_paged_prefill_tree / mm_kv_move_rows", "tree-masked attention")
_VERIFY = ("mm_verify_greedy", "mm_argmax_rows / mm_verify_greedy", "draft verification")
_SAMPLE = ("mm_sample_rows", "mm_sample_rows", "the sampler")
_LOGPROB = ("mm_logprob_rows", "mm_logprob_rows", "token log-probabilities")
_LOGITS = ("mm_process_logits", "mm_process_logits", "logits processing")
_SPEC = ("mm_spec_sample_rows", "mm_spec_sample_rows", "speculative sampling")
_KVSTEP = ("mm_kv_step", "mm_kv_step", "device steps of the page table")
_TOKENS = ("mm_ngram_draft", "mm_token_step / mm_ngram_draft", "the token history on the device")
_RANDOM = ("mm_uniform_rows", "mm_uniform_rows", "seeded uniform numbers")
_SHARED = ("mm_paged_decode_shared", "mm_paged_decode_shared", "shared-prefix decode")


def _kv_bytes(kv_data):
    """an fp8 cache held as torch.float8_e4m3fn, seen as the uint8 tensor the ops take: the same bytes, OCP e4m3fn codes"""
    return kv_data.view(torch.uint8) if isinstance(kv_data, torch.Tensor) and kv_data.dtype is torch.float8_e4m3fn else kv_data


def _kv_geometry(kv_data, kv_param, index):
    """(dtype code, max_pages, L, Hkv, P, kv_data as the C ABI takes it) of a cache, recognised by its shape; int4: uint8
    [max_pages, L, 2, Hkv, P, 64] + fp16 params [..., P, 2]; fp8: uint8 (or torch.float8_e4m3fn, viewed as uint8) [max_pages, L, 2, Hkv,
    P, 128] + the same fp16 params; bf16: bf16 [max_pages, L, 2, Hkv, P, 128] and kv_param None."""
    if kv_param is None:
        if not _ok(kv_data, torch.bfloat16, index):
            _check_tensor(kv_data, "kv_data", torch.bfloat16)
            raise RuntimeError(f"kv_data must be on cuda:{index}")
        if kv_data.dim() != 6 or kv_data.size(2) != 2 or kv_data.size(5) != 128:
            raise RuntimeError("bf16 kv_data (kv_param None) must be [max_pages, L, 2, Hkv, P, 128]; an int4 cache ([..., 64] uint8) and an "
                               "fp8 cache ([..., 128] uint8 / float8_e4m3fn) need their fp16 kv_param")
        kind = _lib.MM_KV_BF16
    else:
        kv_data = _kv_bytes(kv_data)
        if not (_ok(kv_data, torch.uint8, index) and _ok(kv_param, torch.float16, index)):
            _check_tensor(kv_data, "kv_data", torch.uint8)
            _check_tensor(kv_param, "kv_param", torch.float16, kv_data.device)
            raise RuntimeError(f"kv_data / kv_param must be on cuda:{index}")
        if kv_data.dim() != 6 or kv_data.size(2) != 2 or kv_data.size(5) not in (64, 128):
            raise RuntimeError("kv_data with a kv_param must be [max_pages, L, 2, Hkv, P, 64] uint8 (int4) or [max_pages, L, 2, Hkv, P, 128] "
                               "uint8 / float8_e4m3fn (fp8); a bf16 cache [max_pages, L, 2, Hkv, P, 128] takes kv_param None")
        if tuple(kv_param.shape) != tuple(kv_data.shape[:5]) + (2,):
            raise RuntimeError("kv_param must be [max_pages, L, 2, Hkv, P, 2] fp16, matching kv_data")
        kind = _lib.MM_KV_INT4 if kv_data.size(5) == 64 else _lib.MM_KV_FP8_E4M3
    max_pages, L, _, Hkv, P, _ = kv_data.shape
    return kind, max_pages, L, Hkv, P, kv_data


def _cache(kv_data, kv_param, dev=None):
    """(device, dtype code, max_pages, L, Hkv, P, kv_data as the C ABI takes it) of a cache that has to lie on `dev`; None: on the
    device it is found on (an op without a query)"""
    if kv_param is not None:
        kv_data = _kv_bytes(kv_data)
    if dev is None:
        if not (isinstance(kv_data, torch.Tensor) and kv_data.is_cuda):
            _check_tensor(kv_data, "kv_data", torch.uint8 if kv_param is not None else torch.bfloat16)
        dev = kv_data.device
    return (dev, *_kv_geometry(kv_data, kv_param, dev.index))


def _page_table(kv_indptr, kv_indices, last_page_len, dev):
    _tensor(kv_indptr, "kv_indptr", torch.int32, dev)
    _tensor(kv_indices, "kv_indices", torch.int32, dev)
    _tensor(last_page_len, "last_page_len", torch.int32, dev)
    B = last_page_len.numel()
    if kv_indptr.numel() != B + 1:
        raise RuntimeError("kv_indptr must have B + 1 entries (B = last_page_len.numel())")
    return B


def _kv_args(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, layer_idx, q=None):
    """The common checks of the cache ops that take a page table and a layer: (device, B, Hkv, the C arguments kv_data .. batch that
    every entry point takes in this order).  The device is q's (bf16, contiguous); an append has no q and takes the cache's."""
    dev, kind, max_pages, L, Hkv, P, kv_data = _cache(kv_data, kv_param, _lead(q, "q", torch.bfloat16) if q is not None else None)
    B = _page_table(kv_indptr, kv_indices, last_page_len, dev)
    layer_idx = int(layer_idx)
    if not 0 <= layer_idx < L:
        raise RuntimeError(f"layer_idx {layer_idx} outside the cache's {L} layers")
    return dev, B, Hkv, (_ptr(kv_data), _opt(kv_param), kind, max_pages, L, layer_idx, Hkv, P, 128,
                         _ptr(kv_indptr), _ptr(kv_indices), _ptr(last_page_len), B)


def _query_heads(q, Hkv, B=None):
    """Hq of the query an attention wrapper takes: [B, Hq, 128] for decode, [T, Hq, 128] (B None) for prefill, Hq a multiple of Hkv"""
    if q.dim() != 3 or q.size(2) != 128 or (B is not None and q.size(0) != B):
        raise RuntimeError(f"q must be [B = {B}, Hq, 128] bf16" if B is not None else "q must be [T, Hq, 128] bf16, T = qo_indptr[-1]")
    return _head_groups(q.size(1), Hkv)


def _head_groups(Hq, Hkv):
    if Hq % Hkv:
        raise RuntimeError(f"the {Hq} query heads are not a multiple of the cache's {Hkv} kv heads")
    return Hq


def _kv_workspace(workspace, need, dev):
    """(the split-KV scratch, which the caller holds across the launch, its two C arguments): allocated when `need` bytes are wanted and
    none was passed"""
    if not need:
        return None, (None, 0)
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
    if (not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or workspace.device != dev
            or not workspace.is_contiguous() or workspace.numel() * workspace.element_size() < need):
        raise RuntimeError(f"workspace must be a contiguous device tensor of at least {need} bytes on {dev}")
    return workspace, (_ptr(workspace), workspace.numel() * workspace.element_size())


def _sm_scale(sm_scale):
    scale = float(sm_scale) if sm_scale is not None else 128 ** -0.5
    if not scale > 0:
        raise ValueError("sm_scale must be positive")
    return scale


def kv_append(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, k, v, append_indptr, layer_idx):
    """Write T new tokens' K and V (bf16 [T, Hkv, 128]) into layer `layer_idx` of a paged cache, in place.

    Not an export of the reference module (its append_kv_i4 / _f16 take K/V already quantized and one head count).  The page table
    (kv_indptr [B + 1], kv_indices, last_page_len [B], int32) already counts the new tokens; append_indptr [B + 1] splits the T tokens
    among the sequences, each sequence's go to its last positions.  kv_param None: bf16 cache (a copy); otherwise int4 codes + fp16
    (scale, zero) by the rule of quantize_int_group(x, 4, 128), or -- kv_data [..., 128] uint8 / float8_e4m3fn -- e4m3 codes with a
    power-of-two scale per row and zero = 0 (include/micromix_hip.h, MM_KV_FP8_E4M3).  Runs on the current stream, capture-safe.
    """
    lib = _lib.load()
    dev, B, Hkv, kv_args = _kv_args(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, layer_idx)
    _tensor(append_indptr, "append_indptr", torch.int32, dev)
    _tensor(k, "k", torch.bfloat16, dev)
    _tensor(v, "v", torch.bfloat16, dev)
    if k.dim() != 3 or k.shape != v.shape or k.size(1) != Hkv or k.size(2) != 128:
        raise RuntimeError(f"k and v must both be [T, {Hkv}, 128] bf16")
    if append_indptr.numel() != B + 1:
        raise RuntimeError("append_indptr must have B + 1 entries")
    _launch("kv_append", dev, lib.mm_kv_append, *kv_args, _ptr(k), _ptr(v), _ptr(append_indptr), k.size(0), _stream_ptr(dev))


def kv_copy_pages(kv_data, kv_param, src_pages, dst_pages, rows=None):
    """Copy token rows [0, rows[i]) of page src_pages[i] to page dst_pages[i] of a paged cache, for every layer, K and V, every head, in
    place; returns None.  rows None: whole pages.  Bytes only (codes and, for int4 / fp8, the fp16 params): no dequantization.

    src_pages, dst_pages, rows: int32 device tensors of one length.  A pair whose page index lies outside the cache, with src == dst or
    with rows <= 0 is skipped; rows above the page size count as the page size.  The destination pages must be pairwise distinct and
    none of them a source of the same call (include/micromix_hip.h, mm_kv_copy_pages).  What PagedKVCache.extend calls before a sequence
    writes into a partly filled page it shares.  Runs on the current stream, capture-safe."""
    lib = _lib.load()
    dev, kind, max_pages, L, Hkv, P, kv_data = _cache(kv_data, kv_param)
    for n, t in (("src_pages", src_pages), ("dst_pages", dst_pages), ("rows", rows)):
        if t is not None:
            if _tensor(t, n, torch.int32, dev).dim() != 1 or t.numel() != src_pages.numel():
                raise RuntimeError("src_pages, dst_pages and rows must be one-dimensional and of one length")
    _launch("kv_copy_pages", dev, lib.mm_kv_copy_pages, _ptr(kv_data), _opt(kv_param), kind, max_pages, L, Hkv, P, 128, _ptr(src_pages),
            _ptr(dst_pages), _opt(rows), src_pages.numel(), _stream_ptr(dev))


def kv_move_rows(kv_data, kv_param, kv_indptr, kv_indices, move_indptr, src_pos, dst_pos):
    """Within each sequence of a paged cache, move token rows from one logical position to another, for every layer, K and V, every
    head, in place; returns None.  Bytes only (codes and, for int4 / fp8, the fp16 params): no dequantization.

    Sequence b's moves are m in [move_indptr[b], move_indptr[b + 1]): the row at position src_pos[m] goes to position dst_pos[m], a
    position being row pos % P of page kv_indices[kv_indptr[b] + pos // P].  All sources of a sequence are read before any of its
    destinations is written, so a destination may be another move's source -- what packing the accepted path of a tree draft down to
    contiguous positions needs (PagedKVCache.accept).  At most 64 moves per sequence are performed; a move with src == dst, a position
    outside the pages the sequence lists or a page index outside the cache is skipped.  The destinations of a sequence must be pairwise
    distinct, and no page written may be listed by another sequence with moves in the call (include/micromix_hip.h, mm_kv_move_rows).
    move_indptr [B + 1], src_pos, dst_pos: int32 device tensors.  Runs on the current stream, capture-safe."""
    lib = _lib_with(*_TREE)
    dev, kind, max_pages, L, Hkv, P, kv_data = _cache(kv_data, kv_param)
    for n, t in (("kv_indptr", kv_indptr), ("kv_indices", kv_indices), ("move_indptr", move_indptr), ("src_pos", src_pos), ("dst_pos", dst_pos)):
        if _tensor(t, n, torch.int32, dev).dim() != 1:
            raise RuntimeError(f"{n} must be one-dimensional")
    B = kv_indptr.numel() - 1
    if B < 0 or move_indptr.numel() != B + 1:
        raise RuntimeError("kv_indptr and move_indptr must both have B + 1 entries")
    if src_pos.numel() != dst_pos.numel():
        raise RuntimeError("src_pos and dst_pos must be of one length")
    _launch("kv_move_rows", dev, lib.mm_kv_move_rows, _ptr(kv_data), _opt(kv_param), kind, max_pages, L, Hkv, P, 128, _ptr(kv_indptr),
            _ptr(kv_indices), B, _ptr(move_indptr), _ptr(src_pos), _ptr(dst_pos), src_pos.numel(), _stream_ptr(dev))


def kv_step_state_ints(batch, max_pages, pages_per_seq):
    """int32 entries of the state `kv_step` works on (include/micromix_kvstep.h states the layout): MM_KV_STEP_HEADER_INTS + 3 * batch +
    max_pages + batch * pages_per_seq; 0 for arguments `kv_step` refuses"""
    return int(_lib_with(*_KVSTEP).mm_kv_step_state_ints(int(batch), int(max_pages), int(pages_per_seq)))


def kv_step(state, max_pages, pages_per_seq, page_size, max_seq_len, next_new, num_next_tokens, kv_indptr, kv_indices, last_page_len,
            append_indptr, *, keep=None, depths=None, token_pos=None):
    """One step of the paged cache's allocator on the device: every sequence is shortened behind the tokens it keeps of those last
    announced, the pages past them return to the free stack, next_new[b] tokens are announced and get pages, and kv_indptr, kv_indices,
    last_page_len, append_indptr (and token_pos) are rewritten in place; returns None.  What PagedKVCache's accept + extend compute on
    the host, page numbers included (include/micromix_kvstep.h states the rule, the layout of `state` and the MM_KV_STEP_* statuses).

    state: int32 [kv_step_state_ints(B, max_pages, pages_per_seq)], B = next_new.numel() <= MM_KV_STEP_MAX_BATCH.  keep: None (every
    announced token stays: plain decode), int32 [B], or int32 [B, S] whose column 0 counts -- `verify_greedy`'s result as it is.
    num_next_tokens: a host int, what next_new has to sum to (the T of the following appends).  depths: int32 [num_next_tokens], a new
    token's distance from the committed ones (None: chains); token_pos: int32 [num_next_tokens] or None, receives each new token's
    position, its cos / sin row.  A step that cannot be taken (no page left, a sequence past max_seq_len, a count outside its range, ...)
    changes nothing but state[0], its status, and state[3]; every later call then does nothing until the host rewrites the state.  The
    call itself does not fail for that: nothing is read on the host.  All tensors int32 on one device.  Runs on the current stream,
    capture-safe."""
    lib = _lib_with(*_KVSTEP)
    dev = _lead(state, "state", torch.int32)
    B = _tensor(next_new, "next_new", torch.int32, dev).numel()
    for n, t in (("state", state), ("next_new", next_new), ("kv_indptr", kv_indptr), ("kv_indices", kv_indices), ("last_page_len", last_page_len),
                 ("append_indptr", append_indptr), ("depths", depths), ("token_pos", token_pos)):
        if t is not None and _tensor(t, n, torch.int32, dev).dim() != 1:
            raise RuntimeError(f"{n} must be one-dimensional")
    max_pages, pages_per_seq, page_size, max_seq_len, T = int(max_pages), int(pages_per_seq), int(page_size), int(max_seq_len), int(num_next_tokens)
    if min(max_pages, pages_per_seq, page_size, max_seq_len) < 1 or T < 0:
        raise ValueError("max_pages, pages_per_seq, page_size and max_seq_len must be positive and num_next_tokens non-negative")
    most = _lib.KV_STEP["MM_KV_STEP_MAX_BATCH"]
    if B > most:
        raise RuntimeError(f"kv_step takes at most {most} sequences, got {B}")
    if state.numel() < _lib.KV_STEP["MM_KV_STEP_HEADER_INTS"] + 3 * B + max_pages + B * pages_per_seq:
        raise RuntimeError(f"state must hold kv_step_state_ints({B}, {max_pages}, {pages_per_seq}) entries, got {state.numel()}")
    if kv_indptr.numel() != B + 1 or append_indptr.numel() != B + 1 or last_page_len.numel() != B:
        raise RuntimeError("kv_indptr and append_indptr must have B + 1 entries and last_page_len B (B = next_new.numel())")
    stride = 0
    if keep is not None:
        _tensor(keep, "keep", torch.int32, dev)
        if keep.dim() not in (1, 2) or keep.size(0) != B or keep.numel() == 0 and B:
            raise RuntimeError(f"keep must be int32 [{B}] or [{B}, S] with the count in column 0")
        stride = keep.size(1) if keep.dim() == 2 else 1
    for n, t in (("depths", depths), ("token_pos", token_pos)):
        if t is not None and t.numel() != T:
            raise RuntimeError(f"{n} must have num_next_tokens = {T} entries")
    if depths is not None and token_pos is None:
        raise RuntimeError("depths without token_pos: the positions have nowhere to go")
    _launch("kv_step", dev, lib.mm_kv_step, _ptr(state), B, max_pages, pages_per_seq, page_size, max_seq_len, _opt(keep), stride, _ptr(next_new),
            T, _opt(depths), _ptr(kv_indptr), _ptr(kv_indices), kv_indices.numel(), _ptr(last_page_len), _ptr(append_indptr), _opt(token_pos),
            _stream_ptr(dev))


NgramDraft = namedtuple("NgramDraft", ["draft_tok", "root_tok", "cand_tok", "match_len", "row_seq", "row_total_len"])


def _token_state(tokens, total_len, what):
    """(device, batch, ld_tok) of the token history `token_step` and `ngram_draft` share; on the CPU the checks the device path makes"""
    if not isinstance(tokens, torch.Tensor):
        raise TypeError(f"{what}: tokens must be a torch.int32 tensor [batch, ld_tok]")
    if tokens.is_cuda:
        dev = _lead(tokens, "tokens", torch.int32)
    else:
        dev = tokens.device
        if tokens.dtype is not torch.int32 or not tokens.is_contiguous():
            raise TypeError(f"{what}: tokens must be a contiguous torch.int32 tensor [batch, ld_tok]")
    if tokens.dim() != 2 or tokens.size(1) < 1:
        raise RuntimeError(f"tokens must be int32 [batch, ld_tok] with ld_tok >= 1, got {list(tokens.shape)}")
    B, ld = tokens.shape
    if ld > _lib.TOKENS["MM_TOKENS_MAX_LD"] or B > _lib.TOKENS["MM_TOKENS_MAX_BATCH"]:
        raise RuntimeError(f"{what} takes at most {_lib.TOKENS['MM_TOKENS_MAX_BATCH']} sequences of {_lib.TOKENS['MM_TOKENS_MAX_LD']} tokens, got {[B, ld]}")
    _ints(total_len, "total_len", dev, (B,))
    return dev, B, ld


def _ints(t, name, dev, shape=None, new=None):
    """an int32 array of the token ops on `dev`, CPU or device: checked as _tensor checks it, or -- None with `new` -- a new one"""
    if t is None and new is not None:
        return torch.empty(new, dtype=torch.int32, device=dev)
    if dev.type != "cpu":
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        return _tensor(t, name, torch.int32, dev, shape, "int32 {0}, got {1}")
    if not isinstance(t, torch.Tensor) or t.dtype is not torch.int32 or t.device != dev or not t.is_contiguous():
        raise TypeError(f"{name} must be a contiguous torch.int32 tensor on {dev}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{name} must be int32 {list(shape)}, got {list(t.shape)}")
    return t


def _clamp(x, lo, hi):
    return lo if x < lo else hi if x > hi else x


def token_step(tokens, total_len, finished, result, target_tok, qo_indptr, root_tok, max_total, *, stop_tok=None, kv_state=None,
               emitted=None):
    """Commit one verified step into the token history, on the device: the tokens the step generated -- target_tok along the accepted
    path, the bonus last -- are appended to tokens[b] at total_len[b] until a stop token (kept, finished[b] = 1) or the sequence's
    limit min(max_total[b], ld_tok) (finished[b] = 2); returns `emitted`, int32 [B], how many each sequence committed.
    include/micromix_tokens.h states the rule.

    tokens int32 [B, ld_tok], total_len and finished int32 [B]: the state, the layout `process_logits` reads, updated in place.
    result: `verify_greedy`'s, int32 [B, 66]; target_tok int32 [T], qo_indptr int32 [B + 1] and root_tok int32 [B]: what went into it.
    max_total int32 [B]; stop_tok int32 [B, n <= 64] or None, entries < 0 unused; kv_state: `kv_step`'s state or None -- once its
    status is non-zero the whole call writes nothing (call this after `verify_greedy` and BEFORE the step's `kv_step` /
    `step_launch`); emitted: int32 [B] or None (a new one: pass it under capture).  A finished sequence, a prompt chunk (more than
    64 rows, or root_tok[b] < 0) and a sequence whose path is empty are left alone.  Every array is a device tensor that only the kernel
    reads: capture-safe, on the current stream.  On CPU tensors the same rule runs in plain Python over lists."""
    dev, B, ld = _token_state(tokens, total_len, "token_step")
    _ints(finished, "finished", dev, (B,))
    stride = _lib.MM_VERIFY_STRIDE
    _ints(result, "result", dev, (B, stride))
    if _ints(target_tok, "target_tok", dev).dim() != 1:
        raise RuntimeError("target_tok must be one-dimensional")
    T = target_tok.numel()
    _ints(qo_indptr, "qo_indptr", dev, (B + 1,))
    _ints(root_tok, "root_tok", dev, (B,))
    _ints(max_total, "max_total", dev, (B,))
    n_stop = 0
    if stop_tok is not None:
        _ints(stop_tok, "stop_tok", dev)
        most = _lib.TOKENS["MM_TOKENS_MAX_STOP"]
        if stop_tok.dim() != 2 or stop_tok.size(0) != B or not 1 <= stop_tok.size(1) <= most:
            raise RuntimeError(f"stop_tok must be int32 [{B}, n] with 1 <= n <= {most}, got {list(stop_tok.shape)}")
        n_stop = stop_tok.size(1)
    if kv_state is not None and _ints(kv_state, "kv_state", dev).numel() < 1:
        raise RuntimeError("kv_state must be kv_step's state")
    emitted = _ints(emitted, "emitted", dev, (B,), new=(B,))
    if dev.type == "cpu":
        return _token_step_host(tokens, total_len, finished, result, target_tok, qo_indptr, root_tok, max_total, stop_tok, kv_state, emitted)
    _launch("token_step", dev, _lib_with(*_TOKENS).mm_token_step, _ptr(tokens), ld, B, _ptr(total_len), _ptr(finished), _ptr(result), stride,
            _ptr(target_tok), T, _ptr(qo_indptr), _ptr(root_tok), _ptr(max_total), _opt(stop_tok), n_stop, _opt(kv_state), _ptr(emitted),
            _stream_ptr(dev))
    return emitted


def _token_step_host(tokens, total_len, finished, result, target_tok, qo_indptr, root_tok, max_total, stop_tok, kv_state, emitted):
    """the rule of mm_token_step (include/micromix_tokens.h) in plain words, on CPU tensors"""
    if kv_state is not None and int(kv_state.reshape(-1)[0]) != 0:
        return emitted                                           # the sticky failure of kv_step: nothing at all is written
    B, ld = tokens.shape
    target, qo, T = target_tok.tolist(), qo_indptr.tolist(), target_tok.numel()
    for b, row in enumerate(result.tolist()):
        q0 = _clamp(qo[b], 0, T)
        n, k, N, m = _clamp(qo[b + 1], 0, T) - q0, row[0], int(total_len[b]), 0
        path = row[2:2 + max(k, 0)]
        if (int(finished[b]) == 0 and 1 <= n <= 64 and int(root_tok[b]) >= 0 and 1 <= k <= n and N >= 0
                and all(0 <= i < n for i in path)):
            made = [target[q0 + i] for i in path]
            limit = min(int(max_total[b]), ld)
            c = min(k, max(0, limit - N))
            stops = set(t for t in stop_tok[b].tolist() if t >= 0) if stop_tok is not None else set()
            hit = [i for i in range(c) if made[i] in stops]
            m = hit[0] + 1 if hit else c
            if m:
                tokens[b, N:N + m] = torch.tensor(made[:m], dtype=torch.int32)
            total_len[b] = N + m
            if hit:
                finished[b] = _lib.TOKENS["MM_TOKENS_STOPPED"]
            elif N + m >= limit:
                finished[b] = _lib.TOKENS["MM_TOKENS_LENGTH"]
        emitted[b] = m
    return emitted


def ngram_draft_workspace_bytes(batch, ld_tok):
    """bytes of workspace `ngram_draft` needs for a history [batch, ld_tok]: 4 per part of MM_NGRAM_CHUNK tokens of every sequence; 0
    when a history is one part, and for arguments `ngram_draft` refuses"""
    return int(_lib_with(*_TOKENS).mm_ngram_draft_workspace_bytes(int(batch), int(ld_tok)))


def ngram_draft(tokens, total_len, next_indptr, num_tokens, *, min_n=1, max_n=4, draft_tok=None, root_tok=None, cand_tok=None,
                match_len=None, row_seq=None, row_total_len=None, workspace=None):
    """Draft the next chain of every sequence by prompt lookup, on the device: the longest n-gram (at most max_n tokens, at least min_n)
    of the history tokens[b][0 .. total_len[b]) that repeats its end -- the latest among equals -- is continued, periodically where
    the continuation runs into the end; without one the last token is repeated, so the count per step stays fixed.
    include/micromix_tokens.h states the rule.  Returns NgramDraft(draft_tok, root_tok, cand_tok, match_len, row_seq, row_total_len).

    tokens int32 [B, ld_tok], total_len int32 [B]: the state `token_step` keeps.  next_indptr int32 [B + 1]: the next step's qo_indptr
    / append_indptr, at most 64 nodes a sequence; num_tokens: a host int, its last entry (the T of the next step).  1 <= min_n <= max_n
    <= MM_NGRAM_MAX_N = 16.  draft_tok int32 [T]: node 0 of a sequence is its last token, the root, then the draft -- the model's input
    ids and `verify_greedy`'s draft_tok; root_tok int32 [B]: `verify_greedy`'s (-1 for an empty history); cand_tok int32 [T]:
    `chain_candidates`' values, for `spec_sample_rows`' one-hot form; match_len int32 [B]: the n-gram's length, 0 without a match;
    row_seq, row_total_len int32 [T]: what `process_logits` takes for the chain's rows, whose draft tokens are laid into tokens[b] past
    total_len[b] (uncommitted slack that the next `token_step` overwrites).  Outputs that are None are allocated, as is the workspace
    (`ngram_draft_workspace_bytes`, uninitialised): pass them under capture.  Every array is a device tensor that only the kernels
    read: capture-safe, on the current stream.  On CPU tensors the same rule runs in plain Python over lists."""
    dev, B, ld = _token_state(tokens, total_len, "ngram_draft")
    T, min_n, max_n = int(num_tokens), int(min_n), int(max_n)
    most = _lib.TOKENS["MM_NGRAM_MAX_N"]
    if T < 0 or not 1 <= min_n <= max_n <= most:
        raise ValueError(f"ngram_draft needs num_tokens >= 0 and 1 <= min_n <= max_n <= {most}, got {T}, {min_n}, {max_n}")
    _ints(next_indptr, "next_indptr", dev, (B + 1,))
    out = NgramDraft(_ints(draft_tok, "draft_tok", dev, (T,), new=(T,)), _ints(root_tok, "root_tok", dev, (B,), new=(B,)),
                     _ints(cand_tok, "cand_tok", dev, (T,), new=(T,)), _ints(match_len, "match_len", dev, (B,), new=(B,)),
                     _ints(row_seq, "row_seq", dev, (T,), new=(T,)), _ints(row_total_len, "row_total_len", dev, (T,), new=(T,)))
    if dev.type == "cpu":
        return _ngram_draft_host(tokens, total_len, next_indptr, T, min_n, max_n, out)
    lib = _lib_with(*_TOKENS)
    need = int(lib.mm_ngram_draft_workspace_bytes(B, ld))
    workspace, ws_args = _kv_workspace(workspace, need, dev)
    _launch("ngram_draft", dev, lib.mm_ngram_draft, _ptr(tokens), ld, B, _ptr(total_len), _ptr(next_indptr), T, min_n, max_n, _opt(out.draft_tok),
            _ptr(out.root_tok), _opt(out.cand_tok), _ptr(out.match_len), _opt(out.row_seq), _opt(out.row_total_len), *ws_args, _stream_ptr(dev))
    return out


def _ngram_draft_host(tokens, total_len, next_indptr, T, min_n, max_n, out):
    """the rule of mm_ngram_draft (include/micromix_tokens.h) in plain words, on CPU tensors"""
    B, ld = tokens.shape
    nxt = next_indptr.tolist()
    for b in range(B):
        N = _clamp(int(total_len[b]), 0, ld)
        h = tokens[b, :N].tolist()
        best_m, best_e = 0, -1
        for e in range(N - 1):                                   # end positions 0 .. N - 2; later ones win ties
            m = 0
            while m < min(max_n, e + 1) and h[e - m] == h[N - 1 - m]:
                m += 1
            if m and m >= best_m:
                best_m, best_e = m, e
        hit = best_m >= min_n
        last = h[N - 1] if N else 0
        t0 = _clamp(nxt[b], 0, T)
        n = _clamp(nxt[b + 1], 0, T) - t0
        out.root_tok[b] = last if N else -1
        out.match_len[b] = best_m if hit else 0
        if not 1 <= n <= 64:
            continue
        p = N - 1 - best_e
        chain = [last] + [h[best_e + 1 + i % p] if hit else last for i in range(n - 1)]
        out.draft_tok[t0:t0 + n] = torch.tensor(chain, dtype=torch.int32)
        out.cand_tok[t0:t0 + n] = torch.tensor(chain[1:] + [-1], dtype=torch.int32)
        out.row_seq[t0:t0 + n] = b
        out.row_total_len[t0:t0 + n] = torch.tensor([min(N + i, ld) for i in range(n)], dtype=torch.int32)
        slack = chain[1:1 + max(0, min(n - 1, ld - N))]
        if slack:
            tokens[b, N:N + len(slack)] = torch.tensor(slack, dtype=torch.int32)
    return out


def _vector(t, name, dtype, dev, size=None):
    """a one-dimensional array of `uniform_rows` on `dev`, CPU or device, checked as _tensor checks it; returns its length"""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if dev.type != "cpu":
        _tensor(t, name, dtype, dev)
    elif t.dtype is not dtype or t.device != dev or not t.is_contiguous():
        raise TypeError(f"{name} must be a contiguous {dtype} tensor on {dev}")
    if t.dim() != 1 or (size is not None and t.numel() != size):
        raise RuntimeError(f"{name} must be {dtype} [{'n' if size is None else size}], got {list(t.shape)}")
    return t.numel()


def _streams(t, name, dtype, dev, n, rows, ld):
    """an output of `uniform_rows`, [n, rows] with unit stride along the rows and `ld` elements between two streams (None: whatever
    this one has, at least rows); a new dense one for None.  Returns (tensor, ld)"""
    if t is None:
        ld = rows if ld is None else ld
        return torch.empty((n, ld), dtype=dtype, device=dev)[:, :rows], ld
    if not isinstance(t, torch.Tensor) or t.dtype is not dtype or t.device != dev:
        raise TypeError(f"{name} must be a {dtype} tensor on {dev}")
    if tuple(t.shape) != (n, rows) or (rows > 1 and t.stride(1) != 1):
        raise RuntimeError(f"{name} must be {dtype} [{n}, {rows}] with unit stride along the rows, got {list(t.shape)} with strides {list(t.stride())}")
    have = t.stride(0) if n > 1 and rows > 0 else rows if ld is None else ld           # one stream: its stride says nothing
    if have < rows or (ld is not None and have != ld):
        raise RuntimeError(f"{name}: {have} elements between two streams, {'at least ' + str(rows) if ld is None else ld} wanted")
    return t, have


def uniform_rows(seed, pos, *, n=3, sub=None, row_seq=None, domain=0, out=None, bits=False):
    """Uniform numbers for the rows of a sampled step, keyed by the request's seed and the position of the token a row decides: no
    generator state, so what a request draws does not depend on the batch it shares, the row it sits in or the calls before.  Returns
    `out`, fp32 [n, rows]: n streams, each a contiguous [rows] array -- out[0], out[1] (and out[2]) are `spec_sample_rows`' u_accept
    and u_resample (and `sample_rows`' u) without a copy.  With bits=True returns (out, bits), bits int32 [n, rows] holding the 32-bit
    words the numbers were made of.  include/micromix_random.h states the rule.

    seed int64 [batch], one per sequence; pos int32 [rows]: the index in the history at which the token the row decides will be
    committed -- `ngram_draft`'s row_total_len, or total_len for a plain decode step; row_seq int32 [rows]: the row's sequence
    (`ngram_draft`'s row_seq), None: row r is sequence r.  A row whose sequence is outside [0, batch) gets zeros.  sub int32 [batch]
    or None (0): separates the samples or beams of one prompt under one seed; domain, a host integer in [0, 2^32): separates
    consumers (a draft model's sampler from the target's).  1 <= n <= 16, rows <= 2^24.  Row r's words are Philox4x32-10 of counter
    (pos[r], sub[s], block, domain) under key seed[s]; u = (word >> 8) * 2^-24, on the grid the samplers read without clamping.
    out: fp32 [n, rows] or None (a new one: pass it under capture); it may be a view with more than `rows` elements between two
    streams, whose slack is not written.  bits: True, or an int32 [n, rows] tensor with the same distance between two streams.
    Every array is a device tensor that only the kernel reads: capture-safe, on the current stream, no workspace.  On CPU tensors the
    same rule runs in plain Python integers."""
    if not isinstance(seed, torch.Tensor):
        raise TypeError("seed must be a torch.int64 tensor [batch]")
    dev = seed.device
    batch = _vector(seed, "seed", torch.int64, dev)
    rows = _vector(pos, "pos", torch.int32, dev)
    if sub is not None:
        _vector(sub, "sub", torch.int32, dev, batch)
    if row_seq is not None:
        _vector(row_seq, "row_seq", torch.int32, dev, rows)
    most_n, most_rows = _lib.RANDOM["MM_UNIFORM_MAX_N"], _lib.RANDOM["MM_UNIFORM_MAX_ROWS"]
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= most_n:
        raise ValueError(f"uniform_rows needs 1 <= n <= {most_n}, got {n!r}")
    if isinstance(domain, bool) or not isinstance(domain, int) or not 0 <= domain < 1 << 32:
        raise ValueError(f"domain must be an integer in [0, 2^32), got {domain!r}")
    if rows > most_rows:
        raise RuntimeError(f"uniform_rows takes at most {most_rows} rows, got {rows}")
    out, ld = _streams(out, "out", torch.float32, dev, n, rows, None)
    words = None
    if bits is not False:
        words, _ = _streams(None if bits is True else bits, "bits", torch.int32, dev, n, rows, ld)
    if dev.type == "cpu":
        _uniform_rows_host(seed, sub, row_seq, pos, n, domain, out, words)
    else:
        _launch("uniform_rows", dev, _lib_with(*_RANDOM).mm_uniform_rows, _ptr(seed), _opt(sub), batch, _opt(row_seq), _ptr(pos), rows, n, domain,
                _ptr(out), _opt(words), ld, _stream_ptr(dev))
    return out if words is None else (out, words)


def _uniform_rows_host(seed, sub, row_seq, pos, n, domain, out, bits):
    """the rule of mm_uniform_rows (include/micromix_random.h) in plain Python integers, on CPU tensors"""
    mask = 0xFFFFFFFF
    seeds, subs = seed.tolist(), sub.tolist() if sub is not None else None
    seqs = row_seq.tolist() if row_seq is not None else range(pos.numel())
    for r, (s, p) in enumerate(zip(seqs, pos.tolist())):
        words = [0] * n
        if 0 <= s < len(seeds):
            for j in range((n + 3) // 4):
                c = [p & mask, (subs[s] if subs is not None else 0) & mask, j, domain]
                k0, k1 = seeds[s] & mask, seeds[s] >> 32 & mask
                for _ in range(10):
                    a, b = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
                    c = [b >> 32 ^ c[1] ^ k0, b & mask, a >> 32 ^ c[3] ^ k1, a & mask]
                    k0, k1 = k0 + 0x9E3779B9 & mask, k1 + 0xBB67AE85 & mask
                words[4 * j:4 * j + 4] = c[:n - 4 * j]
        for i, w in enumerate(words):
            out[i, r] = (w >> 8) * 2.0 ** -24
            if bits is not None:
                bits[i, r] = w - (w >> 31 << 32)
    return out


def argmax_rows_workspace_bytes(rows, vocab):
    """bytes of workspace `argmax_rows` needs for bf16 logits [rows, vocab]; 0 when a row is one part (vocab <= MM_ARGMAX_CHUNK)"""
    return int(_lib_with(*_VERIFY).mm_argmax_rows_workspace_bytes(int(rows), int(vocab)))


def _logits(logits):
    """(rows, vocab, elements between rows, device) of the bf16 logits `argmax_rows` and `sample_rows` take: unit stride along the
    vocabulary, any row stride >= vocab, nothing copied"""
    if not isinstance(logits, torch.Tensor):
        raise TypeError("logits must be a torch.Tensor")
    if logits.dtype is not torch.bfloat16:
        raise TypeError(f"logits must be torch.bfloat16, got {logits.dtype}")
    if not logits.is_cuda:
        raise RuntimeError("logits must be a device tensor (HIP); the MicroMix ops have no CPU path")
    if logits.dim() != 2 or logits.size(1) < 1:
        raise RuntimeError("logits must be [rows, vocab] with vocab >= 1")
    rows, vocab = logits.shape
    if vocab > 1 and logits.stride(1) != 1:
        raise RuntimeError("logits must have unit stride along the vocabulary (the rows may be any distance >= vocab apart)")
    ld = logits.stride(0) if rows > 1 else vocab
    if ld < vocab:
        raise RuntimeError(f"logits rows overlap: row stride {ld} < vocab {vocab}")
    return rows, vocab, ld, logits.device


def argmax_rows(logits, *, out=None, workspace=None):
    """The index of each row's maximum: logits bf16 [rows, vocab] on the device, last stride 1, any row stride >= vocab (a slice
    logits[:, :V] of a padded lm_head output, at any 2-byte-aligned offset, is taken as it is: nothing is copied).  Returns int32 [rows]
    (`out` when given).  The order is torch.argmax's on the CPU: any NaN is greater than +inf, +0 == -0, the lowest index among equal
    maxima wins.  vocab <= 2^20, rows <= 65535.  workspace: a contiguous device tensor of `argmax_rows_workspace_bytes(rows, vocab)`
    bytes, uninitialised, allocated when needed and not given (under graph capture pass one).  Runs on the current stream,
    capture-safe."""
    lib = _lib_with(*_VERIFY)
    rows, vocab, ld, dev = _logits(logits)
    out = _out(out, "out", torch.int32, dev, (rows,), "int32 {0}")
    workspace, ws_args = _kv_workspace(workspace, argmax_rows_workspace_bytes(rows, vocab), dev)
    _launch("argmax_rows", dev, lib.mm_argmax_rows, _ptr(logits), rows, vocab, ld, _ptr(out), *ws_args, _stream_ptr(dev))
    return out


def sample_rows_workspace_bytes(rows, vocab):
    """bytes of workspace `sample_rows` needs for bf16 logits [rows, vocab]: 3 KiB per part of MM_ARGMAX_CHUNK columns of every row
    and 2 KiB per row"""
    return int(_lib_with(*_SAMPLE).mm_sample_rows_workspace_bytes(int(rows), int(vocab)))


def _row_param(value, name, dtype, rows, dev):
    """a per-row parameter of `sample_rows`: None, a device tensor [rows] of `dtype`, or -- outside graph capture -- a Python number,
    broadcast to one"""
    if value is None:
        return None
    if isinstance(value, torch.Tensor):
        return _tensor(value, name, dtype, dev, (rows,), "{2} {0}, one entry per row")
    if isinstance(value, bool) or not isinstance(value, (int, float)):
        raise TypeError(f"{name} must be None, a number or a {dtype} device tensor [{rows}], got {type(value).__name__}")
    if dtype is torch.int32 and not isinstance(value, int):
        raise TypeError(f"{name} must be an int or a torch.int32 device tensor [{rows}], got {type(value).__name__}")
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"{name}: a Python number would be uploaded during graph capture; pass a {dtype} device tensor [{rows}]")
    if dtype is torch.int32:
        value = min(max(value, -(1 << 31)), (1 << 31) - 1)
    return torch.full((rows,), value, dtype=dtype, device=dev)


def sample_rows(logits, u, *, temperature=None, top_k=None, top_p=None, min_p=None, out=None, workspace=None):
    """One token per row, drawn under temperature, top-k, top-p and min-p: logits bf16 [rows, vocab] on the device as `argmax_rows`
    takes them (any row stride >= vocab, any 2-byte-aligned offset), u fp32 [rows] uniform in [0, 1) -- `torch.rand`, which captures;
    the library draws no random numbers.  Returns int32 [rows] (`out` when given), ready for `verify_greedy` / `verify_launch` as
    target_tok: the accepted path and the bonus token are then distributed as the target model's.

    temperature, top_p, min_p: fp32 [rows], top_k: int32 [rows], device tensors read by the kernels only, so one captured graph serves
    any mix of requests rewritten in place; None: temperature 1, that filter off; a Python number is broadcast to a tensor (outside
    capture only).  Per row: temperature <= 0 or NaN, or a row whose maximum is NaN or infinite, gives exactly `argmax_rows`' answer.
    Otherwise w_i = exp((l_i - max) / T); tokens of equal logit form a class and every filter keeps whole classes in descending
    order: top_k the shortest prefix with >= k tokens (1 <= k < vocab, else off), top_p the shortest prefix with mass >= p times
    top-k's (p < 1; p <= 0 keeps the top class), min_p the classes with w >= q (0 < q <= 1); the kept set is the shortest of the
    three; the answer is the first kept index whose cumulative kept mass exceeds u * Z (include/micromix_hip.h, mm_sample_rows).  The
    result is a function of the inputs alone: the same bits on every run.  vocab <= 2^20, rows <= 65535.  workspace: a contiguous
    device tensor of `sample_rows_workspace_bytes(rows, vocab)` bytes, uninitialised, allocated when not given (under graph capture
    pass one).  Runs on the current stream, capture-safe."""
    lib = _lib_with(*_SAMPLE)
    rows, vocab, ld, dev = _logits(logits)
    if u is None or not isinstance(u, torch.Tensor):
        raise TypeError(f"u must be a torch.float32 device tensor [{rows}] (torch.rand), got {type(u).__name__}")
    u = _row_param(u, "u", torch.float32, rows, dev)
    temperature = _row_param(temperature, "temperature", torch.float32, rows, dev)
    top_k = _row_param(top_k, "top_k", torch.int32, rows, dev)
    top_p = _row_param(top_p, "top_p", torch.float32, rows, dev)
    min_p = _row_param(min_p, "min_p", torch.float32, rows, dev)
    out = _out(out, "out", torch.int32, dev, (rows,), "int32 {0}")
    workspace, ws_args = _kv_workspace(workspace, sample_rows_workspace_bytes(rows, vocab), dev)
    _launch("sample_rows", dev, lib.mm_sample_rows, _ptr(logits), rows, vocab, ld, _ptr(u), _opt(temperature), _opt(top_k), _opt(top_p),
            _opt(min_p), _ptr(out), *ws_args, _stream_ptr(dev))
    return out


def spec_sample_rows_workspace_bytes(rows, vocab):
    """bytes of workspace `spec_sample_rows` needs for bf16 logits [rows, vocab]: 6 KiB + 48 bytes per part of MM_ARGMAX_CHUNK columns
    of every row and about 4.1 KiB per row"""
    return int(_lib_with(*_SPEC).mm_spec_sample_rows_workspace_bytes(int(rows), int(vocab)))


def spec_sample_rows(logits, draft_logits, cand_tok, u_accept, u_resample, *, temperature=None, top_k=None, top_p=None, min_p=None,
                     out=None, accepted=None, workspace=None):
    """Speculative sampling for chain drafts: per row, accept the draft's candidate token with probability min(1, p / q) or redraw
    from norm(max(0, p - q)).  Returns (out, accepted), int32 [rows] each (the tensors given as `out` / `accepted` when given).  `out`
    is ready for `verify_greedy` / `verify_launch` as target_tok: the walk then yields the accepted prefix and, as the bonus token,
    the redraw at the first rejection or the plain sample after the leaf -- distributed exactly as the target model's, and a draft
    token survives with probability sum min(p, q) where `sample_rows -> verify_greedy` gives sum p q.

    logits          bf16 [rows, vocab] as `sample_rows` takes them: row r is the target's logits after node r
    draft_logits    bf16 [rows, vocab] (its own row stride and offset; it may be `logits` itself): row r is the draft model's logits
                    cand_tok[r] was drawn from.  None: one-hot drafts (n-gram, prompt lookup, greedy drafts), q(x) = 1
    cand_tok        int32 [rows]: the token the draft proposed for the next position (`chain_candidates`); < 0 or >= vocab: none
    u_accept, u_resample   fp32 [rows] uniform in [0, 1) (`torch.rand`): the library draws no random numbers
    temperature, top_k, top_p, min_p   as `sample_rows`; the SAME per-row parameters shape p and q, so the draft must have been
                    sampled under the request's parameters (by `sample_rows` from `draft_logits`: then q is bit for bit what it was
                    drawn from)
    accepted[r]     1 accepted, 0 rejected (out[r] is the redraw, never cand_tok[r]), -1 no candidate (out[r] is bit for bit
                    `sample_rows(logits, u_resample, ...)`).  A greedy row (temperature <= 0, ...) gives `argmax_rows`' answer and
                    1 / 0 as it equals the candidate
    p and q are the kept distributions of `sample_rows` as integer masses; the accept test and the residual are formed exactly in
    128-bit integers (include/micromix_spec.h), so the result is a function of the inputs alone.  Chains only: a row has one
    candidate.  For a tree draft `sample_rows` -> `verify_greedy` stays the recommendation.  vocab <= 2^20, rows <= 65535.
    workspace: a contiguous device tensor of `spec_sample_rows_workspace_bytes(rows, vocab)` bytes, uninitialised, allocated when not
    given (under graph capture pass one).  Runs on the current stream, capture-safe."""
    lib = _lib_with(*_SPEC)
    rows, vocab, ld, dev = _logits(logits)
    draft_ld = vocab
    if draft_logits is not None:
        try:
            drows, dvocab, draft_ld, ddev = _logits(draft_logits)
        except (TypeError, RuntimeError) as e:
            raise type(e)(str(e).replace("logits", "draft_logits")) from None
        if (drows, dvocab) != (rows, vocab) or ddev != dev:
            raise RuntimeError(f"draft_logits must be bf16 [{rows}, {vocab}] on {dev}, got {list(draft_logits.shape)} on {ddev}")
    if isinstance(cand_tok, torch.Tensor) and cand_tok.dtype is torch.int64:
        raise TypeError("cand_tok must be torch.int32, got torch.int64: convert it with cand_tok.to(torch.int32)")
    if not isinstance(cand_tok, torch.Tensor):
        raise TypeError(f"cand_tok must be a torch.int32 device tensor [{rows}], got {type(cand_tok).__name__}")
    _tensor(cand_tok, "cand_tok", torch.int32, dev, (rows,), "{2} {0}, one entry per row")
    for name, u in (("u_accept", u_accept), ("u_resample", u_resample)):
        if not isinstance(u, torch.Tensor):
            raise TypeError(f"{name} must be a torch.float32 device tensor [{rows}] (torch.rand), got {type(u).__name__}")
        _tensor(u, name, torch.float32, dev, (rows,), "{2} {0}, one entry per row")
    temperature = _row_param(temperature, "temperature", torch.float32, rows, dev)
    top_k = _row_param(top_k, "top_k", torch.int32, rows, dev)
    top_p = _row_param(top_p, "top_p", torch.float32, rows, dev)
    min_p = _row_param(min_p, "min_p", torch.float32, rows, dev)
    out = _out(out, "out", torch.int32, dev, (rows,), "int32 {0}")
    accepted = _out(accepted, "accepted", torch.int32, dev, (rows,), "int32 {0}")
    workspace, ws_args = _kv_workspace(workspace, spec_sample_rows_workspace_bytes(rows, vocab), dev)
    _launch("spec_sample_rows", dev, lib.mm_spec_sample_rows, _ptr(logits), ld, _opt(draft_logits), draft_ld, rows, vocab, _ptr(cand_tok),
            _ptr(u_accept), _ptr(u_resample), _opt(temperature), _opt(top_k), _opt(top_p), _opt(min_p), _ptr(out), _ptr(accepted), *ws_args,
            _stream_ptr(dev))
    return out, accepted


def chain_candidates(draft_tok, qo_indptr, *, out=None):
    """The candidates `spec_sample_rows` takes for chain drafts laid out as `verify_greedy` takes them: cand[t] = draft_tok[t + 1]
    inside a sequence -- the draft token of node t's child -- and -1 on each sequence's last row (the leaf: its row gives the plain
    sample).  draft_tok int32 [T], qo_indptr int32 [B + 1] with qo_indptr[0] = 0 and qo_indptr[B] = T; returns int32 [T] (`out`
    when given).  An empty sequence, the first one included, touches no row.  Torch index arithmetic on the tensors' own device with
    shapes that depend on T and B alone: nothing is read on the host, so it is capture-safe (under capture pass `out`)."""
    for n, t in (("draft_tok", draft_tok), ("qo_indptr", qo_indptr)):
        if not isinstance(t, torch.Tensor) or t.dtype is not torch.int32 or t.dim() != 1:
            raise TypeError(f"{n} must be a one-dimensional torch.int32 tensor")
    if qo_indptr.device != draft_tok.device or qo_indptr.numel() < 1:
        raise RuntimeError("qo_indptr must have B + 1 >= 1 entries on draft_tok's device")
    T = draft_tok.numel()
    if out is None:
        out = torch.empty_like(draft_tok)
    elif not isinstance(out, torch.Tensor) or out.dtype is not torch.int32 or out.shape != draft_tok.shape or out.device != draft_tok.device:
        raise RuntimeError(f"out must be int32 [{T}] on {draft_tok.device}")
    if T == 0:
        return out
    ends = qo_indptr[1:].to(torch.int64)
    # the last row of every non-empty sequence; an empty one points at the spare entry T, which is dropped
    last = torch.where(ends > qo_indptr[:-1], ends - 1, T).clamp_(0, T)
    is_last = torch.zeros(T + 1, dtype=torch.bool, device=draft_tok.device).index_fill_(0, last, True)
    out[:T - 1].copy_(draft_tok[1:])
    out[T - 1:].fill_(-1)
    return out.masked_fill_(is_last[:T], -1)


LogprobRows = namedtuple("LogprobRows", ["logprob", "rank", "lse", "top_idx", "top_logprob"])


def logprob_rows_workspace_bytes(rows, vocab, top_n=0):
    """bytes of workspace `logprob_rows` needs for bf16 logits [rows, vocab]: at most 24 + 8 top_n bytes per part of MM_ARGMAX_CHUNK
    columns of every row and 8 bytes per row"""
    return int(_lib_with(*_LOGPROB).mm_logprob_rows_workspace_bytes(int(rows), int(vocab), int(top_n)))


def _targets(targets, rows, vocab, dev):
    """the int32 [rows] targets `mm_logprob_rows` takes; int64 (what a tokenizer and torch hand over) is narrowed on the device, a value
    outside [0, vocab) becoming -1, which is ignored like every other such value"""
    if isinstance(targets, torch.Tensor) and targets.dtype is torch.int64:
        _tensor(targets, "targets", torch.int64, dev, (rows,), "int32 or int64 {0}, one entry per row")
        return torch.where((targets >= 0) & (targets < vocab), targets, -1).to(torch.int32)
    if not isinstance(targets, torch.Tensor):
        raise TypeError(f"targets must be None or an int32 or int64 device tensor [{rows}], got {type(targets).__name__}")
    return _tensor(targets, "targets", torch.int32, dev, (rows,), "int32 or int64 {0}, one entry per row")


def logprob_rows(logits, targets=None, *, temperature=None, top_n=0, workspace=None):
    """Log-probabilities of tokens under softmax(logits / T): logits bf16 [rows, vocab] on the device as `argmax_rows` takes them (any
    row stride >= vocab, any 2-byte-aligned offset, nothing copied).  Returns the named tuple (logprob, rank, lse, top_idx,
    top_logprob), with None for what was not asked for:

    logprob, rank   fp32 / int32 [rows], with `targets` (int32 or int64 [rows] on the device): the log-probability of targets[r] and the
                    number of tokens whose logit is greater (0: the target is a greedy token, lm-eval's is_greedy).  A target < 0 or
                    >= vocab is ignored: logprob 0.0, rank -1 (CrossEntropyLoss's ignore_index)
    lse             fp32 [rows], always: log sum_i exp(l_i / T)
    top_idx,        int32 / fp32 [rows, top_n], with 1 <= top_n <= 32: the top_n tokens by descending logit, the lower index first
    top_logprob     among equal ones (column 0 is `argmax_rows`' answer bit for bit), and their log-probabilities; -1 and -inf
                    beyond the vocabulary

    temperature: fp32 [rows] on the device, a Python number (outside graph capture) or None; None, T <= 0 and NaN all mean 1, so a
    greedy request reports the unscaled distribution.  The distribution is the unfiltered one `sample_rows` draws from -- the same
    integer masses, summed exactly -- and the logarithm is taken in fp64 of that sum, so the result is a function of the inputs
    alone: the same bits on every run.  A row whose maximum is NaN or infinite gives NaN values (torch.log_softmax's answer) and the
    same integers (include/micromix_logprob.h).  vocab <= 2^20, rows <= 65535.  workspace: a contiguous device tensor of
    `logprob_rows_workspace_bytes(rows, vocab, top_n)` bytes, uninitialised, allocated when not given (under graph capture pass
    one).  Runs on the current stream, capture-safe."""
    lib = _lib_with(*_LOGPROB)
    rows, vocab, ld, dev = _logits(logits)
    if isinstance(top_n, bool) or not isinstance(top_n, int) or not 0 <= top_n <= 32:
        raise ValueError(f"top_n must be an int in 0 .. 32, got {top_n!r}")
    logprob = rank = top_idx = top_logprob = None
    if targets is not None:
        targets = _targets(targets, rows, vocab, dev)
        logprob = torch.empty((rows,), dtype=torch.float32, device=dev)
        rank = torch.empty((rows,), dtype=torch.int32, device=dev)
    temperature = _row_param(temperature, "temperature", torch.float32, rows, dev)
    lse = torch.empty((rows,), dtype=torch.float32, device=dev)
    if top_n:
        top_idx = torch.empty((rows, top_n), dtype=torch.int32, device=dev)
        top_logprob = torch.empty((rows, top_n), dtype=torch.float32, device=dev)
    workspace, ws_args = _kv_workspace(workspace, logprob_rows_workspace_bytes(rows, vocab, top_n), dev)
    _launch("logprob_rows", dev, lib.mm_logprob_rows, _ptr(logits), rows, vocab, ld, _opt(targets), _opt(temperature), _opt(logprob),
            _opt(rank), _ptr(lse), top_n, _opt(top_idx), _opt(top_logprob), *ws_args, _stream_ptr(dev))
    return LogprobRows(logprob, rank, lse, top_idx, top_logprob)


def cross_entropy(logits, labels, *, ignore_index=-100, reduction="mean"):
    """nn.CrossEntropyLoss's forward for bf16 logits [rows, vocab] and integer labels [rows] on the device, as an fp32 tensor: a scalar
    for reduction "mean" (over the rows that are not ignored; NaN when all are, as torch gives) and "sum", [rows] for "none" (0 where
    ignored).  A label equal to `ignore_index`, negative or >= vocab is ignored.

    The per-row term is -`logprob_rows(logits, labels).logprob`: no [rows, vocab] fp32 tensor is formed.  The reduction over the rows
    is a torch fp64 sum on the device, rounded to fp32 once.  The reference's evaluation applies nn.CrossEntropyLoss to the bf16
    logits themselves, which rounds the mean loss to bf16's 8 bits of mantissa; this does not.  More than 65535 rows are taken in
    slices.  Not capture-safe (it allocates and narrows the labels)."""
    if reduction not in ("mean", "sum", "none"):
        raise ValueError(f"reduction must be 'mean', 'sum' or 'none', got {reduction!r}")
    rows, vocab, ld, dev = _logits(logits)
    if not isinstance(labels, torch.Tensor) or labels.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"labels must be an int32 or int64 device tensor [{rows}]")
    _tensor(labels, "labels", labels.dtype, dev, (rows,), "{2} {0}, one entry per row")
    labels = torch.where(labels == ignore_index, -1, labels)
    step = _lib.MM_ARGMAX_MAX_ROWS
    nll = torch.cat([-logprob_rows(logits[i:i + step], labels[i:i + step]).logprob for i in range(0, rows, step)]) if rows else \
        torch.zeros((0,), dtype=torch.float32, device=dev)
    if reduction == "none":
        return nll
    total = nll.sum(dtype=torch.float64)
    if reduction == "mean":
        total = total / ((labels >= 0) & (labels < vocab)).sum()
    return total.to(torch.float32)


def _rows_of(t, name, dtype, rows, dev, min_cols=0):
    """an optional [rows, n] array of `process_logits` (n >= min_cols; rows None: one row or more), as _tensor checks it; returns
    (t, n)"""
    if t is None:
        return None, 0
    lead = "n_seq" if rows is None else rows
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be None or a {dtype} device tensor [{lead}, n], got {type(t).__name__}")
    _tensor(t, name, dtype, dev)
    if t.dim() != 2 or (t.size(0) < 1 if rows is None else t.size(0) != rows) or t.size(1) < max(min_cols, 1):
        raise RuntimeError(f"{name} must be {dtype} [{lead}, n] with n >= {max(min_cols, 1)}, got {list(t.shape)}")
    return t, t.size(1)


def _row_array(t, name, dtype, rows, dev):
    """an optional per-row device array of `process_logits`: a tensor only, since the kernel is what reads it"""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be None or a {dtype} device tensor [{rows}], got {type(t).__name__}")
    return _tensor(t, name, dtype, dev, (rows,), "{2} {0}, one entry per row")


def process_logits(logits, *, out=None, tokens=None, prompt_len=None, total_len=None, row_seq=None, repetition_penalty=None,
                   frequency_penalty=None, presence_penalty=None, bias_idx=None, bias_val=None, allowed_mask=None):
    """What a request does to the logits before a token is picked, in one launch: repetition, frequency and presence penalties over a
    token history, a bias list and an allowed-token bitmask.  logits bf16 [rows, vocab] on the device as `argmax_rows` takes them (any
    row stride >= vocab, any 2-byte-aligned offset).  Returns `out`, bf16 [rows, vocab]: a new tensor for None, `logits` itself for
    the in-place form, or any tensor or strided view of that shape that does not otherwise overlap the logits; columns beyond vocab
    of a padded `out` are not written.  `sample_rows`, `argmax_rows` and `logprob_rows` take the result as it is.

    tokens          int32 [n_seq, ld_tok]: the token history of every sequence, prompt first; ids outside [0, vocab) (padding) are
                    ignored.  With it prompt_len and total_len, int32 [rows]: row r reads tokens[s][0 .. prompt_len[r]) as its prompt
                    and [prompt_len[r] .. total_len[r]) as its output (both clamped to the buffer), s = row_seq[r] (int32 [rows]) or
                    r.  The lengths belong to the row and the buffer to the sequence: n samples of one prompt share a buffer, and
                    the rows of a chain draft read one buffer under total_len = base + i + 1.  s outside [0, n_seq): no history
    repetition_penalty   fp32 [rows]: a token seen in prompt or output has its logit x divided by it (x < 0: multiplied), HF's rule;
                    a value that is not finite and > 0 is off
    frequency_penalty, presence_penalty   fp32 [rows]: a token that occurs c > 0 times in the output loses frequency * c, then
                    presence (vLLM's and OpenAI's rule); NaN is off
    bias_idx, bias_val   int32 / fp32 [rows, n]: bias_val[r][j] is added to token bias_idx[r][j]; of several entries for one token
                    the last (highest j) counts; ids outside [0, vocab) are padding; -inf bans a token
    allowed_mask    int32 [rows, >= ceil(vocab / 32)]: xgrammar's bitmask; a token whose bit is clear becomes -inf
    Every one of them is a device tensor that only the kernel reads, so a captured graph serves requests rewritten in place; None
    is off.  The steps run in the order above, each a correctly rounded fp32 operation on (float)logit, the result rounded to bf16
    once (include/micromix_logits.h): a function of the inputs alone, the same bits on every run.  vocab <= 2^20, rows <= 65535,
    ld_tok <= 2^24, n <= 2^20.  No workspace, nothing allocated but a missing `out`.  Runs on the current stream, capture-safe."""
    lib = _lib_with(*_LOGITS)
    rows, vocab, ld_in, dev = _logits(logits)
    if out is None:
        out = torch.empty((rows, vocab), dtype=torch.bfloat16, device=dev)
        ld_out = vocab
    elif out is logits:
        ld_out = ld_in
    else:
        try:
            orows, ovocab, ld_out, odev = _logits(out)
        except (TypeError, RuntimeError) as e:
            raise type(e)(str(e).replace("logits", "out")) from None
        if (orows, ovocab) != (rows, vocab) or odev != dev:
            raise RuntimeError(f"out must be bf16 [{rows}, {vocab}] on {dev}, got {list(out.shape)} on {odev}")
    tokens, ld_tok = _rows_of(tokens, "tokens", torch.int32, None, dev)
    n_seq = tokens.size(0) if tokens is not None else 0
    per_row = dict(prompt_len=prompt_len, total_len=total_len, row_seq=row_seq, repetition_penalty=repetition_penalty,
                   frequency_penalty=frequency_penalty, presence_penalty=presence_penalty)
    if tokens is None:
        given = [n for n, v in per_row.items() if v is not None]
        if given:
            raise RuntimeError(f"{given[0]} needs tokens: the history it is applied over")
    elif prompt_len is None or total_len is None:
        raise RuntimeError(f"{'prompt_len' if prompt_len is None else 'total_len'} is required with tokens (int32 [{rows}])")
    prompt_len = _row_array(prompt_len, "prompt_len", torch.int32, rows, dev)
    total_len = _row_array(total_len, "total_len", torch.int32, rows, dev)
    row_seq = _row_array(row_seq, "row_seq", torch.int32, rows, dev)
    repetition_penalty = _row_array(repetition_penalty, "repetition_penalty", torch.float32, rows, dev)
    frequency_penalty = _row_array(frequency_penalty, "frequency_penalty", torch.float32, rows, dev)
    presence_penalty = _row_array(presence_penalty, "presence_penalty", torch.float32, rows, dev)
    if (bias_idx is None) != (bias_val is None):
        raise RuntimeError(f"{'bias_val' if bias_val is None else 'bias_idx'} is missing: bias_idx and bias_val come together")
    bias_idx, n_bias = _rows_of(bias_idx, "bias_idx", torch.int32, rows, dev)
    bias_val, n_val = _rows_of(bias_val, "bias_val", torch.float32, rows, dev)
    if n_val != n_bias:
        raise RuntimeError(f"bias_val must be fp32 {[rows, n_bias]} like bias_idx, got {list(bias_val.shape)}")
    allowed_mask, ld_mask = _rows_of(allowed_mask, "allowed_mask", torch.int32, rows, dev, (vocab + 31) // 32)
    _launch("process_logits", dev, lib.mm_process_logits, _ptr(logits), rows, vocab, ld_in, _ptr(out), ld_out, _opt(tokens), ld_tok, n_seq,
            _opt(row_seq), _opt(prompt_len), _opt(total_len), _opt(repetition_penalty), _opt(frequency_penalty), _opt(presence_penalty),
            _opt(bias_idx), _opt(bias_val), n_bias, _opt(allowed_mask), ld_mask, _stream_ptr(dev))
    return out


def verify_greedy(target_tok, draft_tok, root_tok, qo_indptr, kv_indptr, last_page_len, page_size, *, tree_mask=None, result=None,
                  move_src=None, move_dst=None):
    """Greedy (exact-match) verification of tree or chain drafts, one wave per sequence; returns (result, move_src, move_dst).

    Sequence b has the n = qo_indptr[b + 1] - qo_indptr[b] draft nodes of rows qo_indptr[b] .. : draft_tok[t] is a node's token,
    target_tok[t] the token the target model picks after it (`argmax_rows` or `sample_rows` of its logits), root_tok[b] the token
    picked after the last committed one.  tree_mask: the int64 words of `paged_prefill(tree_mask=)` -- a node's parent is the highest set
    bit below its own -- or None for chains.  Starting from root_tok[b], the walk takes the lowest-numbered child of the node just taken
    whose token is the one wanted, until there is none.  result int32 [B, 66]: [0] the path's length k, [1] the bonus token (the
    target's choice after the last node taken; root_tok[b] when nothing matched), [2 : 2 + k] the path, the rest -1.  A sequence with
    n > 64 or root_tok[b] < 0 is a prompt chunk and keeps all: [0] = n, [1] = target_tok of its last row (-1 for n = 0), path entries -1.
    move_src, move_dst int32 [T], laid over qo_indptr: pass them on as `kv_move_rows(..., move_indptr=qo_indptr, move_src, move_dst)`
    to pack each path down to the positions base_b .. base_b + k - 1 (base_b = len_b - n, len_b from kv_indptr / last_page_len /
    page_size).  Every element of the three outputs is written.  All tensors are int32 on one device (token ids as int64 are refused:
    convert them with .to(torch.int32)).  Runs on the current stream, capture-safe (include/micromix_hip.h, mm_verify_greedy)."""
    lib = _lib_with(*_VERIFY)
    ints = (("target_tok", target_tok), ("draft_tok", draft_tok), ("root_tok", root_tok), ("qo_indptr", qo_indptr), ("kv_indptr", kv_indptr),
            ("last_page_len", last_page_len))
    for n, t in ints:                                      # what torch.argmax and a tokenizer hand over: say what to do about it
        if isinstance(t, torch.Tensor) and t.dtype is torch.int64:
            raise TypeError(f"{n} must be torch.int32, got torch.int64: convert it with {n}.to(torch.int32)")
    if not (isinstance(target_tok, torch.Tensor) and target_tok.is_cuda):
        _check_tensor(target_tok, "target_tok", torch.int32)
    dev = target_tok.device
    for n, t in ints:
        if _tensor(t, n, torch.int32, dev).dim() != 1:
            raise RuntimeError(f"{n} must be one-dimensional")
    T, B = target_tok.numel(), root_tok.numel()
    if draft_tok.numel() != T:
        raise RuntimeError("target_tok and draft_tok must be of one length")
    if qo_indptr.numel() != B + 1 or kv_indptr.numel() != B + 1 or last_page_len.numel() != B:
        raise RuntimeError("qo_indptr and kv_indptr must have B + 1 entries and last_page_len B (B = root_tok.numel())")
    page_size = int(page_size)
    if page_size < 1:
        raise ValueError("page_size must be positive")
    if tree_mask is not None:
        _tensor(tree_mask, "tree_mask", torch.int64, dev, (T,), "int64 {0}, one word per row")
    result = _out(result, "result", torch.int32, dev, (B, _lib.MM_VERIFY_STRIDE), "int32 {0}")
    move_src = _out(move_src, "move_src", torch.int32, dev, (T,), "int32 {0}")
    move_dst = _out(move_dst, "move_dst", torch.int32, dev, (T,), "int32 {0}")
    _launch("verify_greedy", dev, lib.mm_verify_greedy, _ptr(target_tok), _ptr(draft_tok), _ptr(root_tok), _opt(tree_mask), _ptr(qo_indptr), T,
            _ptr(kv_indptr), _ptr(last_page_len), page_size, B, _ptr(result), _ptr(move_src), _ptr(move_dst), _stream_ptr(dev))
    return result, move_src, move_dst


def _token_rows(t, name, heads):
    """(heads, token stride in elements) of q / k / v given as [T, H, 128] or [T, H * 128] whose rows lie contiguous within a token.
    Stride 0: any stride will do (at most one token); None: the tensor has to be copied (rows not contiguous, an odd stride, a
    misaligned pointer)"""
    if t.dim() == 3 and t.size(2) == 128:
        H, inner = t.size(1), t.stride(2) == 1 and (t.size(1) == 1 or t.stride(1) == 128)
    elif t.dim() == 2 and t.size(1) % 128 == 0 and t.size(1):
        H, inner = t.size(1) // 128, t.stride(1) == 1
    else:
        raise RuntimeError(f"{name} must be [T, H, 128] or [T, H * 128] bf16")
    if heads is not None and H != heads:
        raise RuntimeError(f"{name} has {H} heads, the cache has {heads}")
    stride = t.stride(0) if t.size(0) > 1 else 0
    ok = inner and (stride == 0 or stride >= H * 128) and stride % 2 == 0 and t.data_ptr() % 4 == 0
    return H, (stride if ok else None)


def rope_kv_append(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, q, k, v, cos, sin, append_indptr, layer_idx):
    """RoPE on q and k, then `kv_append` of (rotated k, v), in one launch; returns the rotated q, bf16 [T, Hq, 128] contiguous.

    q, k, v: bf16 [T, H, 128] or [T, H * 128].  Views of one packed [T, (Hq + 2 Hkv) * 128] projection (what FusedQLinear returns) are
    read in place; so are any three tensors with one common token stride.  Otherwise they are packed into one buffer first (one copy).
    cos, sin: bf16 [T, 128], or HF's [1, T, 128] / [bsz, q_len, 128] (flattened): row i belongs to flat token i; a row stride is honoured.
    RoPE is HF's apply_rotary_pos_emb in bf16 arithmetic, q * cos + rotate_half(q) * sin with every op rounded to bf16, bit for bit
    (include/micromix_hip.h, mm_rope_kv_append).  The cache receives exactly what kv_append(rope(k), v) writes; q is rotated for every
    token.  Page table, append_indptr and the three cache kinds (int4, fp8 e4m3, bf16) as in `kv_append`.  Runs on the current stream,
    capture-safe.
    """
    lib = _lib.load()
    dev, B, Hkv, kv_args = _kv_args(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, layer_idx)
    _tensor(append_indptr, "append_indptr", torch.int32, dev)
    if append_indptr.numel() != B + 1:
        raise RuntimeError("append_indptr must have B + 1 entries")
    for n, t in (("q", q), ("k", k), ("v", v), ("cos", cos), ("sin", sin)):
        if not (isinstance(t, torch.Tensor) and t.dtype is torch.bfloat16 and t.is_cuda and t.get_device() == dev.index):
            _check_tensor(t, n, torch.bfloat16, dev)      # contiguity is not asked of these five
    Hq, sq = _token_rows(q, "q", None)
    _, sk = _token_rows(k, "k", Hkv)
    _, sv = _token_rows(v, "v", Hkv)
    T = q.size(0)
    if k.size(0) != T or v.size(0) != T:
        raise RuntimeError("q, k and v must hold the same T tokens")
    _head_groups(Hq, Hkv)
    strides = {sq, sk, sv} - {0}
    if None in strides or len(strides) > 1 or max(strides, default=Hq * 128) < Hq * 128:
        packed = torch.cat([q.reshape(T, Hq * 128), k.reshape(T, Hkv * 128), v.reshape(T, Hkv * 128)], dim=1)
        q, k, v = packed[:, : Hq * 128], packed[:, Hq * 128: (Hq + Hkv) * 128], packed[:, (Hq + Hkv) * 128:]
        strides = {(Hq + 2 * Hkv) * 128}
    sq = max(strides, default=Hq * 128)
    if cos.shape != sin.shape or cos.dim() not in (2, 3) or cos.size(-1) != 128 or cos.numel() != T * 128:
        raise RuntimeError(f"cos and sin must both be [T = {T}, 128] (or [bsz, q_len, 128] with bsz * q_len = T) bf16")
    cos, sin = cos.reshape(T, 128), sin.reshape(T, 128)
    sc = cos.stride(0) if T > 1 else 128
    if not (cos.stride(1) == 1 and sin.stride(1) == 1 and (T <= 1 or sin.stride(0) == sc) and sc >= 128 and sc % 2 == 0
            and cos.data_ptr() % 4 == 0 and sin.data_ptr() % 4 == 0):
        cos, sin, sc = cos.contiguous(), sin.contiguous(), 128
    q_rot = torch.empty((T, Hq, 128), dtype=torch.bfloat16, device=dev)
    _launch("rope_kv_append", dev, lib.mm_rope_kv_append, *kv_args, _ptr(q), _ptr(k), _ptr(v), sq, Hq, _ptr(cos), _ptr(sin), sc,
            _ptr(append_indptr), T, _ptr(q_rot), _stream_ptr(dev))
    return q_rot


def _window(window):
    """HF's sliding_window as the C ABI takes it: None or 0 is no window (the un-windowed entry points), W >= 1 a window of W tokens"""
    window = 0 if window is None else int(window)
    if window < 0:
        raise ValueError("window must be None, 0 (no window) or a positive token count")
    return window


def paged_decode_workspace_bytes(B, Hq, Hkv, max_seq_len, window=None):
    """bytes of fp32 scratch paged_decode needs for this bound and window (0: one launch, no workspace)"""
    window = _window(window)
    if not window:
        return int(_lib.load().mm_paged_decode_workspace_bytes(int(B), int(Hq), int(Hkv), int(max_seq_len)))
    return int(_lib.load().mm_paged_decode_window_workspace_bytes(int(B), int(Hq), int(Hkv), int(max_seq_len), window))


def _max_seq_len(max_seq_len):
    max_seq_len = int(max_seq_len)
    if max_seq_len < 0:
        raise RuntimeError("max_seq_len must be >= 0")
    return max_seq_len


def paged_decode(q, kv_data, kv_param, kv_indptr, kv_indices, last_page_len, layer_idx, max_seq_len, sm_scale=None, workspace=None, *,
                 window=None):
    """Single-token GQA attention over layer `layer_idx` of a paged cache: q bf16 [B, Hq, 128] -> o bf16 [B, Hq, 128].

    Query head h reads kv head h // (Hq / Hkv) (HF repeat_kv), every cached token, softmax in fp32 with sm_scale (default 1/sqrt(128));
    a sequence of length 0 gives zeros.  `max_seq_len` bounds the sequence lengths; the split over the tokens depends on it (and B,
    Hq, Hkv) only, so a captured graph stays valid while the sequences grow up to it.  `workspace` (uint8 / any device tensor of at
    least paged_decode_workspace_bytes(...) bytes) is allocated here when None -- pass one when capturing a graph.
    `window` = W (HF's sliding_window; None or 0: none): the query attends the last W tokens of its sequence, its own included.  Only
    these tokens are read, the split is laid over W tokens, and page-table entries below the window may be -1.
    The cache is int4, fp8 (e4m3) or bf16, told apart as in `kv_append`; over an fp8 cache the result equals, bit for bit, that over a
    bf16 cache holding the dequantized values.
    """
    lib = _lib.load()
    window = _window(window)
    dev, B, Hkv, kv_args = _kv_args(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, layer_idx, q)
    Hq = _query_heads(q, Hkv, B)
    max_seq_len = _max_seq_len(max_seq_len)
    need = paged_decode_workspace_bytes(B, Hq, Hkv, max_seq_len, window) if B else 0
    workspace, ws_args = _kv_workspace(workspace, need, dev)
    o = torch.empty((B, Hq, 128), dtype=torch.bfloat16, device=dev)
    args = (_ptr(q), *kv_args, Hq, max_seq_len, _sm_scale(sm_scale), *ws_args, _ptr(o))
    if window:
        _launch("paged_decode", dev, lib.mm_paged_decode_window, *args, _stream_ptr(dev), window)
    else:
        _launch("paged_decode", dev, lib.mm_paged_decode, *args, _stream_ptr(dev))
    return o


def paged_decode_shared_workspace_bytes(B, Hq, Hkv, max_shared_len, max_suffix_len):
    """bytes of fp32 scratch paged_decode_shared needs for these bounds: the partials of its prefix and tail chunks (never 0 for B > 0
    and sizes the call takes; 0 for sizes it refuses)"""
    return int(_lib_with(*_SHARED).mm_paged_decode_shared_workspace_bytes(int(B), int(Hq), int(Hkv), int(max_shared_len), int(max_suffix_len)))


def paged_decode_shared(q, kv_data, kv_param, kv_indptr, kv_indices, last_page_len, layer_idx, group_indptr, group_members, shared_len,
                        max_shared_len, max_suffix_len, sm_scale=None, workspace=None, *, out=None):
    """`paged_decode` for a batch in which groups of sequences hold their leading pages in common: q bf16 [B, Hq, 128] -> o bf16
    [B, Hq, 128], the same function (every sequence attends all of its tokens), within the same budget but not the same bits.

    The shared tokens of a group are walked once per slab of 16 // (Hq // Hkv) members instead of once per member; each sequence's own
    tail is walked as in `paged_decode`.  group_indptr [B + 1], group_members [B], shared_len [B]: int32 device tensors.  Group j is
    group_members[group_indptr[j] : group_indptr[j + 1]], trailing unused groups are empty (group_indptr[j] = B), group_members is a
    permutation of range(B), and shared_len[b] -- the same for every member of a group, at most each member's length, any value, not
    only multiples of the page size -- counts the leading tokens b has on the same pages as its group (include/micromix_hip.h,
    mm_paged_decode_shared, also for what happens when the tensors break the rules: wrong results for those sequences, no access outside
    the tensors).  `PagedKVCache.share_groups()` derives one grouping from a page table; a caller who knows better (a beam tree whose
    branches share different depths) passes its own.
    `max_shared_len` bounds the shared counts, `max_suffix_len` the tails; the launches depend on them (and B, Hq, Hkv) only, so a
    captured graph stays valid while lengths and groups change within them.  `workspace` (at least
    paged_decode_shared_workspace_bytes(...) bytes; always needed) is allocated here when None -- pass one when capturing a graph.
    `out`: a bf16 [B, Hq, 128] tensor to write instead of a new one.  No sliding window.
    """
    lib = _lib_with(*_SHARED)
    dev, B, Hkv, kv_args = _kv_args(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, layer_idx, q)
    Hq = _query_heads(q, Hkv, B)
    for n, t, size in (("group_indptr", group_indptr, B + 1), ("group_members", group_members, B), ("shared_len", shared_len, B)):
        if _tensor(t, n, torch.int32, dev).dim() != 1 or t.numel() != size:
            raise RuntimeError(f"{n} must be a one-dimensional int32 tensor of {size} entries (B = {B})")
    max_shared_len, max_suffix_len = int(max_shared_len), int(max_suffix_len)
    if min(max_shared_len, max_suffix_len) < 0 or max(max_shared_len, max_suffix_len) > 1 << 29:
        raise RuntimeError("max_shared_len and max_suffix_len must lie in [0, 2^29]")
    need = paged_decode_shared_workspace_bytes(B, Hq, Hkv, max_shared_len, max_suffix_len) if B and Hq // Hkv <= 16 else 0
    workspace, ws_args = _kv_workspace(workspace, need, dev)
    out = _out(out, "out", torch.bfloat16, dev, (B, Hq, 128), "{0} bf16")
    _launch("paged_decode_shared", dev, lib.mm_paged_decode_shared, _ptr(q), *kv_args, Hq, _ptr(group_indptr), _ptr(group_members),
            _ptr(shared_len), max_shared_len, max_suffix_len, _sm_scale(sm_scale), *ws_args, _ptr(out), _stream_ptr(dev))
    return out


def paged_prefill_workspace_bytes(T, B, Hq, Hkv, max_seq_len, window=None):
    """bytes of fp32 scratch paged_prefill needs for T query tokens over B sequences within max_seq_len, under `window` (0: one launch,
    no workspace)"""
    window = _window(window)
    if not window:
        return int(_lib.load().mm_paged_prefill_workspace_bytes(int(T), int(B), int(Hq), int(Hkv), int(max_seq_len)))
    return int(_lib.load().mm_paged_prefill_window_workspace_bytes(int(T), int(B), int(Hq), int(Hkv), int(max_seq_len), window))


def paged_prefill(q, kv_data, kv_param, kv_indptr, kv_indices, last_page_len, qo_indptr, layer_idx, max_seq_len, sm_scale=None,
                  workspace=None, *, window=None, tree_mask=None):
    """Causal GQA attention of T new query tokens over layer `layer_idx` of a paged cache: q bf16 [T, Hq, 128] -> o bf16 [T, Hq, 128].

    qo_indptr (int32 [B + 1], qo_indptr[B] = T) splits the queries among the sequences, as kv_append's append_indptr does; pass the
    same array.  The page table already counts the new tokens, and the mask is aligned bottom-right: sequence b's j-th new token sits
    at position len_b - n_b + j and attends positions 0 .. that one.  Softmax in fp32 with sm_scale (default 1/sqrt(128)).
    `max_seq_len` bounds the sequence lengths; the grid and the split over the tokens depend on it (and T, B, Hq, Hkv) only, so a
    captured graph stays valid over later steps with the same T.  `workspace` (any contiguous device tensor of at least
    paged_prefill_workspace_bytes(...) bytes) is allocated here when None -- pass one when capturing a graph.
    `window` = W (HF's sliding_window; None or 0: none): the token at position p attends positions max(0, p - W + 1) .. p; the kv tiles
    below a query tile's windows are not read, and page-table entries below every window may be -1.
    `tree_mask` (int64 [T] device tensor, one word per query token; None: the causal mask): verification of a tree draft.  With
    base_b = len_b - n_b, sequence b's j-th new token attends every position below base_b and new slot base_b + i exactly when i <= j
    and bit i of its word is set (bits above j are ignored; set bit j for a token to attend itself).  A sequence with more than 64 new
    tokens ignores its words and is attended causally.  Words (2 << j) - 1 give the bits of the causal call.  No window form: `window`
    together with `tree_mask` is a ValueError.  The tensor is read by the kernel only, so a captured graph replays with other trees
    written into it.  `PagedKVCache.tree_mask` builds the words from parent indices.
    The cache is int4, fp8 (e4m3) or bf16, told apart as in `kv_append`; fp8 runs p.V on bf16(p * scale_v) times the codes, as int4.
    """
    lib = _lib.load() if tree_mask is None else _lib_with(*_TREE)
    window = _window(window)
    if window and tree_mask is not None:
        raise ValueError("paged_prefill has no sliding-window form of the tree mask: pass window or tree_mask, not both")
    dev, B, Hkv, kv_args = _kv_args(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, layer_idx, q)
    _tensor(qo_indptr, "qo_indptr", torch.int32, dev)
    if qo_indptr.numel() != B + 1:
        raise RuntimeError("qo_indptr must have B + 1 entries (B = last_page_len.numel())")
    Hq = _query_heads(q, Hkv)
    T = q.size(0)
    if tree_mask is not None:
        if _tensor(tree_mask, "tree_mask", torch.int64, dev).dim() != 1 or tree_mask.numel() != T:
            raise RuntimeError(f"tree_mask must be a one-dimensional int64 tensor of T = {T} words")
    max_seq_len = _max_seq_len(max_seq_len)
    need = paged_prefill_workspace_bytes(T, B, Hq, Hkv, max_seq_len, window) if B and T else 0
    workspace, ws_args = _kv_workspace(workspace, need, dev)
    o = torch.empty((T, Hq, 128), dtype=torch.bfloat16, device=dev)
    args = (_ptr(q), _ptr(qo_indptr), T, *kv_args, Hq, max_seq_len, _sm_scale(sm_scale), *ws_args, _ptr(o))
    if tree_mask is not None:
        _launch("paged_prefill", dev, lib.mm_paged_prefill_tree, *args, _stream_ptr(dev), _ptr(tree_mask))
    elif window:
        _launch("paged_prefill", dev, lib.mm_paged_prefill_window, *args, _stream_ptr(dev), window)
    else:
        _launch("paged_prefill", dev, lib.mm_paged_prefill, *args, _stream_ptr(dev))
    return o
