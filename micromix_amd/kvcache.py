"""A small paged KV cache for decode on top of `mixedgemm.kv_append` / `mixedgemm.paged_decode`.

    cache = PagedKVCache(num_layers=32, num_kv_heads=8, page_size=16, max_pages=4096, batch=4, kind="int4")
    cache.extend(1)                        # one new token per sequence: pages allocated, page table updated (host side, before a graph)
    for layer in range(32):
        cache.append(layer, k, v)          # k, v bf16 [T, Hkv, 128], T = the tokens extend() announced
        o = cache.attend(layer, q)         # q bf16 [B, Hq, 128] -> o bf16 [B, Hq, 128]
        # or, from the q | k | v projection before RoPE, with HF's bf16 cos / sin rows [T, 128]: one launch instead of RoPE + append
        o = cache.attend(layer, cache.append_rope(layer, q, k, v, cos, sin))

    cache.extend([300, 512, 5])            # several tokens per sequence: a prompt, a chunk of one, a speculative draft
    for layer in range(32):
        cache.append(layer, k, v)          # k, v bf16 [T, Hkv, 128], T = 817
        o = cache.attend_new(layer, q)     # q bf16 [T, Hq, 128] -> o bf16 [T, Hq, 128], causal over each sequence's cache

The page table lives in device tensors of fixed capacity that `extend` rewrites in place, so `append` + `attend` (or `attend_new`) captured once into a
hipGraph replay correctly after later `extend` calls, as long as T stays the same and the sequences stay within the captured
`max_seq_len`.  The allocator is a free list: no eviction, no prefix sharing.
"""
from __future__ import annotations

import torch

from . import mixedgemm

HEAD_DIM = 128


class PagedKVCache:
    def __init__(self, num_layers, num_kv_heads, page_size, max_pages, batch, kind="int4", device="cuda"):
        if kind not in ("int4", "bf16"):
            raise ValueError("kind must be 'int4' or 'bf16'")
        if min(num_layers, num_kv_heads, page_size, max_pages, batch) <= 0:
            raise ValueError("num_layers, num_kv_heads, page_size, max_pages and batch must be positive")
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.num_layers, self.num_kv_heads, self.page_size, self.max_pages, self.batch = num_layers, num_kv_heads, page_size, max_pages, batch
        self.kind, self.device = kind, dev
        shape = (max_pages, num_layers, 2, num_kv_heads, page_size)
        if kind == "int4":
            self.kv_data = torch.zeros(shape + (HEAD_DIM // 2,), dtype=torch.uint8, device=dev)
            self.kv_param = torch.zeros(shape + (2,), dtype=torch.float16, device=dev)
        else:
            self.kv_data = torch.zeros(shape + (HEAD_DIM,), dtype=torch.bfloat16, device=dev)
            self.kv_param = None
        self._free = list(range(max_pages - 1, -1, -1))        # pop() hands out low page numbers first
        self._pages = [[] for _ in range(batch)]
        self.seq_lens = [0] * batch
        i32 = dict(dtype=torch.int32, device=dev)
        self.kv_indptr = torch.zeros((batch + 1,), **i32)
        self.kv_indices = torch.zeros((max_pages,), **i32)     # capacity: every page, so the tensor never moves
        self.last_page_len = torch.zeros((batch,), **i32)
        self.append_indptr = torch.zeros((batch + 1,), **i32)
        self.num_new_tokens = 0
        self._workspace = None
        self._prefill_workspace = None
        self._retired = []

    def _upload(self, new):
        indptr, indices, last = [0], [], []
        for b in range(self.batch):
            indices += self._pages[b]
            indptr.append(len(indices))
            n = self.seq_lens[b]
            last.append(n - (len(self._pages[b]) - 1) * self.page_size if n else 0)
        app = [0]
        for n in new:
            app.append(app[-1] + n)
        self.kv_indptr.copy_(torch.tensor(indptr, dtype=torch.int32))
        if indices:
            self.kv_indices[: len(indices)].copy_(torch.tensor(indices, dtype=torch.int32))
        self.last_page_len.copy_(torch.tensor(last, dtype=torch.int32))
        self.append_indptr.copy_(torch.tensor(app, dtype=torch.int32))
        self.num_new_tokens = app[-1]

    def extend(self, new_tokens_per_seq):
        """Announce the next tokens: an int (the same count for every sequence) or one count per sequence.  Allocates pages and
        rewrites the page table in place (host -> device copies; call it outside graph capture).  The following `append` calls of
        every layer take exactly sum(counts) tokens, sequence by sequence."""
        new = [int(new_tokens_per_seq)] * self.batch if isinstance(new_tokens_per_seq, int) else [int(n) for n in new_tokens_per_seq]
        if len(new) != self.batch or min(new) < 0:
            raise ValueError(f"need {self.batch} non-negative token counts")
        need = [-(-(self.seq_lens[b] + n) // self.page_size) - len(self._pages[b]) for b, n in enumerate(new)]
        if sum(need) > len(self._free):
            raise RuntimeError(f"out of pages: {sum(need)} needed, {len(self._free)} free")
        for b, n in enumerate(new):
            self._pages[b] += [self._free.pop() for _ in range(need[b])]
            self.seq_lens[b] += n
        self._upload(new)

    def reset(self, seq):
        """Empty sequence `seq` and return its pages to the free list (outside graph capture)."""
        self._free += reversed(self._pages[seq])
        self._pages[seq] = []
        self.seq_lens[seq] = 0
        self._upload([0] * self.batch)

    def append(self, layer, k, v):
        """Write the announced tokens' K and V (bf16 [T, Hkv, 128]) of `layer`."""
        if k.dim() != 3 or k.size(0) != self.num_new_tokens:
            raise RuntimeError(f"append expects the {self.num_new_tokens} tokens announced by extend(), got k of shape {tuple(k.shape)}")
        mixedgemm.kv_append(self.kv_data, self.kv_param, self.kv_indptr, self.kv_indices, self.last_page_len, k, v, self.append_indptr, layer)

    def append_rope(self, layer, q, k, v, cos, sin):
        """RoPE + `append` in one launch: rotates q and k (bf16 [T, H, 128] or [T, H * 128], e.g. the views FusedQLinear returns) by the
        bf16 cos / sin rows of the announced tokens ([T, 128] or HF's [bsz, q_len, 128]), writes the rotated K and V of `layer` and returns
        the rotated q, bf16 [T, Hq, 128], for `attend` / `attend_new`.  Bit-equal to HF's bf16 apply_rotary_pos_emb followed by `append`."""
        if q.dim() not in (2, 3) or q.size(0) != self.num_new_tokens:
            raise RuntimeError(f"append_rope expects the {self.num_new_tokens} tokens announced by extend(), got q of shape {tuple(q.shape)}")
        return mixedgemm.rope_kv_append(self.kv_data, self.kv_param, self.kv_indptr, self.kv_indices, self.last_page_len, q, k, v, cos, sin,
                                        self.append_indptr, layer)

    def attend(self, layer, q, max_seq_len=None, sm_scale=None):
        """Decode attention of q (bf16 [B, Hq, 128]) over `layer`.  max_seq_len defaults to the longest sequence now (host
        bookkeeping, no device sync); under graph capture pass the bound the replays will stay within."""
        bound = max(self.seq_lens) if max_seq_len is None else int(max_seq_len)
        need = mixedgemm.paged_decode_workspace_bytes(self.batch, q.size(1), self.num_kv_heads, bound)
        if need and (self._workspace is None or self._workspace.numel() < need):
            if self._workspace is not None:
                self._retired.append(self._workspace)      # a graph captured earlier may still point at it
            self._workspace = torch.empty((need,), dtype=torch.uint8, device=self.device)
        return mixedgemm.paged_decode(q, self.kv_data, self.kv_param, self.kv_indptr, self.kv_indices, self.last_page_len, layer, bound,
                                      sm_scale=sm_scale, workspace=self._workspace if need else None)

    def attend_new(self, layer, q, max_seq_len=None, sm_scale=None):
        """Causal attention of the tokens the last `extend()` announced: q (bf16 [num_new_tokens, Hq, 128], sequence by sequence) over
        `layer`, each new token attending its sequence's cache up to and including itself.  Call it after `append` of the same layer.
        max_seq_len as in `attend`."""
        if q.dim() != 3 or q.size(0) != self.num_new_tokens:
            raise RuntimeError(f"attend_new expects the {self.num_new_tokens} tokens announced by extend(), got q of shape {tuple(q.shape)}")
        bound = max(self.seq_lens) if max_seq_len is None else int(max_seq_len)
        need = mixedgemm.paged_prefill_workspace_bytes(self.num_new_tokens, self.batch, q.size(1), self.num_kv_heads, bound)
        if need and (self._prefill_workspace is None or self._prefill_workspace.numel() < need):
            if self._prefill_workspace is not None:
                self._retired.append(self._prefill_workspace)      # a graph captured earlier may still point at it
            self._prefill_workspace = torch.empty((need,), dtype=torch.uint8, device=self.device)
        return mixedgemm.paged_prefill(q, self.kv_data, self.kv_param, self.kv_indptr, self.kv_indices, self.last_page_len,
                                       self.append_indptr, layer, bound, sm_scale=sm_scale,
                                       workspace=self._prefill_workspace if need else None)
