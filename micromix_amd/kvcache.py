"""A small paged KV cache for decode on top of `mixedgemm.kv_append` / `mixedgemm.paged_decode`.

    cache = PagedKVCache(num_layers=32, num_kv_heads=8, page_size=16, max_pages=4096, batch=4, kind="int4")   # or "bf16", "fp8_e4m3"
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

`kind` is "int4" (the reference's --kv_cache rule: asymmetric, 16 levels per 128-value row), "bf16" (exact, two bytes per value) or
"fp8_e4m3" (OCP e4m3fn codes with a power-of-two scale per row: half the bytes of bf16, relative error at most 2^-4 per value, and
attention that equals, bit for bit, attention over a bf16 cache of the dequantized values).  Nothing else in the class depends on it.

The page table lives in device tensors of fixed capacity that `extend` rewrites in place, so `append` + `attend` (or `attend_new`) captured once into a
hipGraph replay correctly after later `extend` calls, as long as T stays the same and the sequences stay within the captured
`max_seq_len`.  The allocator is a free list with a reference count per page, so sequences can share pages (below).

    cache = PagedKVCache(..., window=4096)  # HF's sliding_window: a token attends the last 4096 positions, its own included

With a window, `attend` / `attend_new` visit only the tiles that hold it, and `extend` evicts: every page whose positions all lie below
what the announced tokens can attend -- below len_b - n_b - W + 1, len_b counting the n_b new tokens (for n_b = 0: below len_b - W, what
a decode query at the last position attends) -- returns to the free list, and its entry in `kv_indices` becomes -1.  The entry stays, so
positions, `seq_lens` and the append slots do not move; a sequence holds at most ceil((W + n_b) / P) + 1 pages, whatever its length,
and a long chat costs the window, not the history.  Without a window nothing is evicted.  `release=False` keeps the pages (the mask
alone), for callers who share pages between sequences.  The page table itself still grows by one entry per page_size tokens:
`max_seq_len` sizes `kv_indices` for batch * ceil(max_seq_len / P) entries up front; past its capacity the tensor is replaced by a
larger one, and a graph captured before that has to be captured again.

    cache.fork(0, 1)                        # sequence 1 = sequence 0, no byte copied: n samples of one prompt, beams, a shared system prompt
    cache.fork(0, 2, length=21)             # ... or its first 21 tokens
    cache.truncate(1, cache.seq_lens[1] - 3)   # drop the last 3 tokens: the rejected part of a speculative draft

Sharing.  `fork` gives `dst` the page list of `src` and raises each page's count; `truncate`, `reset` and the window's release lower
counts, and a page returns to the free list when its last owner lets go.  The rule: a page is written only by a sequence that is its
sole owner.  The only page a sequence ever writes that may already hold tokens is its last one, so `extend` checks exactly that: a
sequence about to receive tokens whose last page is partly filled (in its own view) and counted more than once first takes a fresh
page, swaps it into its list and drops its reference to the old one; the rows it holds there, [0, seq_len % P), are copied by one
`mixedgemm.kv_copy_pages` launch for all such sequences of the call (copy-on-write; on a CPU cache, by slice assignment), on the current
stream before `extend` returns, so before any later `append`.  Full shared pages are never copied, and neither is anything when the
other owners have let go in the meantime.  Tokens past a sequence's length on a page it owns alone are simply overwritten.
With a window, a fork or truncate to `length` is refused (ValueError) when it would keep a released page inside the window of the shorter
sequence -- unless released_pages * P <= max(0, length - W) -- because the -1 entries would silently mask tokens it must attend.
Shared pages are listed once per owner, so the page table can outgrow `max_pages` entries; `max_seq_len` sizes it as above.
Graphs captured earlier stay valid across `fork`, `truncate` and a copying `extend` (the tables are rewritten in place), replayed on a
stream ordered after the `extend`.  `pages_in_use` is the number of pages off the free list.

    o = cache.attend(layer, q, shared=True)    # the same attention; tokens that forked sequences share are read once, not once each

Shared-prefix decode.  `attend(shared=True)` calls `mixedgemm.paged_decode_shared`: the sequences of a group put their queries into the
rows of one matrix operand -- 16 // (Hq // Hkv) sequences to a slab, 4 for Llama-3-8B -- and one walk over the tokens they share serves
the slab; each sequence's own tail is walked as before and a merge launch combines the two.  The result is within the same budget as
`attend()` but not the same bits (the sums run in another order).  The groups come from `share_groups()`, which every table change
(`extend`, `fork`, `truncate`, `reset`) recomputes and writes, in place, into three int32 device tensors of fixed size made in
`__init__` (`group_indptr` [B + 1], `group_members` [B], `shared_len` [B]): a graph captured with `shared=True` stays valid while groups
form and dissolve.  `shared=True` always takes this path, also when nothing is shared -- then it costs three launches where `attend()`
has one or two -- so a graph captured before the first fork needs no second capture.  `share_groups()` puts a sequence into the first
group whose leader lists the same first page and gives the group the number of leading pages on which ALL its members agree (times the
page size, capped at the shortest member): a beam tree whose branches share different depths gets the depth common to the whole tree,
which is correct and not optimal; a caller who wants more passes its own groups to `mixedgemm.paged_decode_shared`.  A cache with a
window refuses `shared=True` (ValueError): every member's window begins elsewhere.  `shared=False`, the default, is the call it was.
Measured (Llama-3-8B heads): 1.2 x faster for 64 samples of a 4 096-token prompt, slower for 8 samples of it, for 64 samples
of 1 024 tokens and when nothing is shared -- take it for many samples of a long prompt.

    cache.extend([21, 0, 5])                               # a tree draft of 21 nodes for sequence 0, a chain of 5 for sequence 2
    mask, depths = cache.tree_mask([parents, None, None])  # parents[i]: -1 (child of the last committed token) or an earlier node
    for layer in range(32):                                # cos / sin row of node i of sequence b: position base_b + depths[b][i]
        o = cache.attend_new(layer, cache.append_rope(layer, q, k, v, cos, sin), tree=mask)
    cache.accept([[1, 6, 13], None, [0, 1]])               # keep one root-to-leaf path per sequence; the rest of the draft is dropped

Tree drafts (Medusa, EAGLE, SpecInfer: candidate continuations that share ancestors, verified in one forward pass).  `extend(n)`
announces the n nodes of a tree in any order that puts a parent before its children; node i goes to slot base + i.  `tree_mask`
turns the parent lists into one 64-bit word per new token -- bit i of node j's word: node i is j or an ancestor of j -- and the
depths; `attend_new(tree=mask)` calls `mixedgemm.paged_prefill(tree_mask=)`, in which a node attends every committed token and the
new slots its word names.  At most 64 nodes per sequence (one word); a sequence given as None is a causal chain of any length, so a
prompt chunk and tree drafts mix in one call.  The mask tensor is read on the device only: a graph captured with `tree=mask` replays
with another tree copied into the same tensor.  A chain's words give the bits `attend_new(layer, q)` gives.
`accept(paths)` is `truncate`'s counterpart for a tree: the rows of the accepted nodes sit in scattered slots base + path[i] and have to
become positions base + i.  One `mixedgemm.kv_move_rows` launch moves them for all sequences and all layers -- every source read before
any destination is written, since packing a path down overwrites slots that are still wanted -- then each sequence is shortened to
base + len(path) as `truncate` would and the tables are uploaded once.  Call it after the last layer's `append`, outside capture; it
refuses (ValueError) when the tables changed since the `extend` (`fork`, `truncate`, `reset`, another `extend`) and a path that is not a
chain from the root under the parents given to `tree_mask`.  No window form: a cache made with `window=` refuses `tree=`.
Measured (Llama-3-8B heads): a 21-node tree in one call is 8 to 16 % faster than its 16 paths as forked sequences and holds
66 pages for 80; with a chain's words the tree kernels are 1.5 to 3 % slower than the causal ones for int4 and bf16, so verify a
chain without `tree=`.

    logits = lm_head(hidden)                               # bf16 [T, vocab], the rows of the announced nodes
    paths, nxt = cache.verify(mixedgemm.argmax_rows(logits), draft_tok, root_tok)     # int32 ids; instead of accept(paths)

Verifying a draft.  Greedy (exact-match) verification picks the path on the device: `mixedgemm.argmax_rows` gives the token the target
model chooses after every node (torch.argmax's order on the CPU: NaN above +inf, the lowest index among equals), and
`verify(target_tok, draft_tok, root_tok)` walks each sequence's tree from `root_tok[b]` -- the token chosen after the last committed
one, the previous step's bonus -- taking the lowest-numbered child whose draft token is the one wanted, until there is none.  It is two
halves.  `verify_launch` runs `mixedgemm.verify_greedy` (one wave per sequence; a node's parent is read from its `tree_mask` word, the
highest bit below its own) and then `mixedgemm.kv_move_rows` straight from the move table the walk wrote, with no host work between or
before them, so `argmax_rows` -> `verify_launch` can close the captured graph of a step; it uses the words of the last `tree_mask`
call, chains without one.  `commit(result)` copies 66 ints per sequence to the host -- the path's length, the bonus token, the path --
and does `accept`'s validation and bookkeeping without launching moves.  A sequence with more than 64 announced tokens or a negative
`root_tok` is a prompt chunk and keeps all its tokens; a cache made with `window=` verifies chains, which have no moves.  A path the
host validation refuses (ValueError) is refused after the rows have moved: the announced rows are then undefined, the committed tokens
untouched, and `truncate(b, base_b)` recovers.  Token ids are int32 (convert torch.argmax's and a tokenizer's int64).
Measured (vocabulary 128 256): `argmax_rows` takes 5 to 9 us for 1 to 64 rows and 61 us for 64 x 21 (71 % of 8 TB/s), 2 to
8 x faster than torch.argmax; `verify_launch` 5 to 6 us for one sequence's 21-node tree in 32 layers, 42 to 48 us for 64.  By the host
clock the whole `verify` is 14 % shorter than ids to the host + a Python walk + `accept` for 64 sequences and no shorter for one:
`commit` still pays `accept`'s bookkeeping and table upload.  What it buys is a step whose device work is one graph.

    cache.extend(counts); cache.tree_mask(parents)         # the first announce on the host: pages, copy-on-write, the tree
    for step in range(8):                                  # ... and then no host bookkeeping: capturable, all 8 steps in one graph
        for layer in range(32):
            o = cache.attend_new(layer, cache.append_rope(layer, q, k, v, cos, sin), max_seq_len=4096, tree=mask)
        result = cache.verify_launch(mixedgemm.argmax_rows(lm_head(hidden)), draft_tok, root_tok)
        token_pos = cache.step_launch(result, counts, max_seq_len=4096, depths=depths)     # commit + the next extend, on the device
    cache.sync()                                           # the host lists catch up: one copy

Device steps.  `step_launch(result, next_counts, max_seq_len=)` is `commit(result)` + `extend(next_counts)` as one capture-safe call of
`mixedgemm.kv_step` (include/micromix_kvstep.h): every sequence is shortened behind the tokens `result` says it keeps (None: all of
them, the plain decode loop), the pages past them go back to a free stack ON THE DEVICE, the next tokens get pages from it, and
`kv_indptr`, `kv_indices`, `last_page_len` and `append_indptr` are rewritten in place -- the tables the host code produces, entry for
entry, page numbers included, because every push and pop lands where the host's sequential loops put it (prefix sums over the
sequences, no atomics).  It returns `token_pos`, the position of every new token: its cos / sin row.  The device state -- lengths, page
lists, the stack -- is one int32 tensor that the host packs and uploads when its own tables changed since the last upload
(`upload_state`, or a `step_launch` outside capture) and reads back with `sync()`, which always copies the state that is on the
device -- a replayed graph moves it without any Python running -- and rebuilds `_pages`, the free list in
the stack's order, the reference counts and `seq_lens`, and announces the last step's tokens again so that `commit` / `accept` can
close it on the host.  While the device is ahead -- after a `step_launch`, and, once one was captured, whenever the 16-byte header of the state says
that a graph has run since the host last looked -- everything that needs the host lists raises RuntimeError naming `sync()`: `extend`,
`fork`, `truncate`, `reset`, `accept`, `commit`, `share_groups`, `pages_in_use`, `seq_lens`, `steps_guaranteed`, and `attend` /
`attend_new` without an explicit `max_seq_len`; `append`, `append_rope`, `attend` / `attend_new` with `max_seq_len`, `tree_mask` and
`verify_launch` work.  `attend(shared=True)` with both bounds keeps working too: a device step never shortens a sequence below the
tokens that were committed when the groups were formed, so the shared prefixes and the group tables stay valid.
A step that cannot be taken -- no page left, a sequence past `max_seq_len`, a keep count outside its range -- changes nothing and
leaves a sticky status; the later steps of a captured graph then do nothing, its appends rewrite slots the sequences already own, and
`sync()` raises naming the step and the status with the host state that of the last good step.  `steps_guaranteed(next_counts,
max_seq_len)` says how many steps cannot fail.  No reference counts exist on the device and none are needed: a dropped page holds
only announced tokens, written by this sequence alone into a page it took for them, so shared pages are never pushed; what has to
hold on entry is that no sequence's partly filled last page is shared (the host `extend` before the first step sees to it, ValueError
otherwise), and steps keep that (`step_launch`).  Out of scope: releasing pages below a window (a cache made with `window=` and
release on refuses), `fork` on the device, counts that change from step to step inside one graph, more than 1 024 sequences.
"""
from __future__ import annotations

import torch

from . import _lib, mixedgemm

HEAD_DIM = 128


class PagedKVCache:
    def __init__(self, num_layers, num_kv_heads, page_size, max_pages, batch, kind="int4", device="cuda", window=None, release=True, max_seq_len=None):
        if kind not in ("int4", "bf16", "fp8_e4m3"):
            raise ValueError("kind must be 'int4', 'bf16' or 'fp8_e4m3'")
        self.window = 0 if window is None else int(window)
        if self.window < 0:
            raise ValueError("window must be None, 0 (no window) or a positive token count")
        self.release = bool(release) and self.window > 0
        if min(num_layers, num_kv_heads, page_size, max_pages, batch) <= 0:
            raise ValueError("num_layers, num_kv_heads, page_size, max_pages and batch must be positive")
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.num_layers, self.num_kv_heads, self.page_size, self.max_pages, self.batch = num_layers, num_kv_heads, page_size, max_pages, batch
        self.kind, self.device = kind, dev
        shape = (max_pages, num_layers, 2, num_kv_heads, page_size)
        if kind in ("int4", "fp8_e4m3"):      # int4: two codes per byte; fp8 (OCP e4m3fn): one; both with fp16 (scale, zero) per row
            self.kv_data = torch.zeros(shape + (HEAD_DIM // 2 if kind == "int4" else HEAD_DIM,), dtype=torch.uint8, device=dev)
            self.kv_param = torch.zeros(shape + (2,), dtype=torch.float16, device=dev)
        else:
            self.kv_data = torch.zeros(shape + (HEAD_DIM,), dtype=torch.bfloat16, device=dev)
            self.kv_param = None
        self._free = list(range(max_pages - 1, -1, -1))        # pop() hands out low page numbers first
        self._pages = [[] for _ in range(batch)]                # -1: a page released below the window; its entry keeps its place
        self._released = [0] * batch                            # leading entries of _pages[b] that are -1
        self._ref = [0] * max_pages                             # entries of _pages that name the page; 0: the page is in _free, once
        self._seq_lens = [0] * batch
        i32 = dict(dtype=torch.int32, device=dev)
        self.kv_indptr = torch.zeros((batch + 1,), **i32)
        # capacity: every page, so the tensor never moves -- unless released entries (which keep their place) outgrow it
        self.kv_indices = torch.zeros((max(max_pages, batch * -(-int(max_seq_len or 0) // page_size)),), **i32)
        self.last_page_len = torch.zeros((batch,), **i32)
        self.append_indptr = torch.zeros((batch + 1,), **i32)
        # the groups of attend(shared=True), one tensor so that a table change costs one more copy: views of fixed size and address
        self._group_table = torch.tensor(list(range(batch + 1)) + list(range(batch)) + [0] * batch, **i32)   # nobody shares yet
        self.group_indptr, self.group_members, self.shared_len = self._group_table.split([batch + 1, batch, batch])
        self._max_shared = self._max_suffix = 0                 # the largest shared count and the longest tail now
        self.num_new_tokens = 0
        self._announced = None                                  # (counts, bases) of the last extend while the tables are still its own
        self._parents = None                                    # what tree_mask was given for them (None: chains)
        self._tree_words = None                                 # tree_mask's words, kept at one address for verify_launch ...
        self._tree_words_live = False                           # ... and whether they describe the tokens announced now
        self._verify_result = torch.zeros((batch, _lib.MM_VERIFY_STRIDE), **i32)
        self._verify_moves = None                               # move_src | move_dst, two halves of one tensor
        self._workspace = None
        self._shared_workspace = None
        self._prefill_workspace = None
        self._retired = []
        # device steps (the module docstring, "Device steps")
        self._ahead = False                                     # the device took steps the host lists have not seen: sync() reads them
        self._state_current = False                             # the packed state on the device equals the host lists
        self._step_state = None                                 # the state of mixedgemm.kv_step, and (max_seq_len, pages_per_seq) it was made for
        self._step_geometry = None
        self._step_counts = self._step_depths = None            # what _next_new and _depths_dev hold
        self._next_new = self._depths_dev = self._token_pos = self._token_pos_view = None    # made by the first step_launch / upload_state
        self._captured = False                                  # a step_launch was captured: a graph replay moves the device unseen
        self._steps_seen = 0                                    # steps_done of the state when the host last wrote or read it
        self._shared_host = [0] * batch                         # shared_len as it was last uploaded

    @property
    def seq_lens(self):
        """tokens per sequence, the announced ones included (host bookkeeping; RuntimeError while the device is ahead: `sync()`)"""
        self._host("seq_lens")
        return self._seq_lens

    @seq_lens.setter
    def seq_lens(self, value):
        self._seq_lens = value

    def _host(self, what):
        """the host lists are current, or RuntimeError.  The Python of a captured step_launch does not run at a replay, so once one
        was captured the state's header is read (16 bytes) to see whether a graph has moved the device since sync() or the upload"""
        if not self._ahead and self._captured and self._state_current:
            status, steps_done = self._step_state[:2].tolist()
            self._ahead = bool(status) or steps_done != self._steps_seen
        if self._ahead:
            raise RuntimeError(f"{what}: the device has taken steps (step_launch) that the host lists have not seen; call sync() first")

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
        if len(indices) > self.kv_indices.numel():
            self._retired.append(self.kv_indices)          # a graph captured earlier may still point at it
            self.kv_indices = torch.zeros((2 * len(indices),), dtype=torch.int32, device=self.device)
        if indices:
            self.kv_indices[: len(indices)].copy_(torch.tensor(indices, dtype=torch.int32))
        self.last_page_len.copy_(torch.tensor(last, dtype=torch.int32))
        self.append_indptr.copy_(torch.tensor(app, dtype=torch.int32))
        self.num_new_tokens = app[-1]
        self._announced = self._parents = None                  # extend sets them again after its upload
        self._tree_words_live = False
        self._state_current = False                             # step_launch packs the lists again
        groups, shared = self.share_groups()
        gptr = [0]
        for grp in groups:
            gptr.append(gptr[-1] + len(grp))
        gptr += [self.batch] * (self.batch + 1 - len(gptr))    # the unused trailing groups are empty
        self._group_table.copy_(torch.tensor(gptr + [b for grp in groups for b in grp] + shared, dtype=torch.int32))
        self._shared_host = shared
        self._max_shared = max(shared)
        self._max_suffix = max(n - c for n, c in zip(self.seq_lens, shared))

    def share_groups(self):
        """(groups, shared): the grouping `attend(shared=True)` uses, from the page lists alone (host only; works on a CPU cache).
        groups: lists of sequence indices that together hold every sequence once; shared[b]: the leading tokens sequence b has on the
        same pages as the rest of its group.  Sequences are taken in index order; b joins the first group whose leader (its first
        member) lists the same page, a real one (>= 0), in entry 0, and opens a group otherwise.  A group shares
        page_size * (leading entries on which all its members agree), capped at its shortest member's length; a group of one shares 0."""
        self._host("share_groups")
        groups = []
        for b, pages in enumerate(self._pages):
            for grp in groups:
                lead = self._pages[grp[0]]
                if pages and lead and pages[0] >= 0 and pages[0] == lead[0]:
                    grp.append(b)
                    break
            else:
                groups.append([b])
        shared = [0] * self.batch
        for grp in groups:
            if len(grp) > 1:
                lists = [self._pages[b] for b in grp]
                n = 0
                while n < min(map(len, lists)) and lists[0][n] >= 0 and all(x[n] == lists[0][n] for x in lists):
                    n += 1
                count = min(n * self.page_size, min(self.seq_lens[b] for b in grp))
                for b in grp:
                    shared[b] = count
        return groups, shared

    @property
    def pages_in_use(self):
        self._host("pages_in_use")
        return self.max_pages - len(self._free)

    def _unref(self, page):
        self._ref[page] -= 1
        if self._ref[page] == 0:
            self._free.append(page)

    def _take(self):
        page = self._free.pop()
        self._ref[page] = 1
        return page

    def _copy_pages(self, pairs):
        """rows [0, r) of page `old` -> page `new` for every (old, new, r): one launch on the current stream"""
        if self.device.type == "cpu":                            # the host tests' path, and the copy rule in plain words
            for old, new, r in pairs:
                self.kv_data[new, :, :, :, :r] = self.kv_data[old, :, :, :, :r]
                if self.kv_param is not None:
                    self.kv_param[new, :, :, :, :r] = self.kv_param[old, :, :, :, :r]
            return
        src, dst, rows = (torch.tensor(c, dtype=torch.int32).to(self.device) for c in zip(*pairs))
        mixedgemm.kv_copy_pages(self.kv_data, self.kv_param, src, dst, rows)

    def extend(self, new_tokens_per_seq):
        """Announce the next tokens: an int (the same count for every sequence) or one count per sequence.  Allocates pages and
        rewrites the page table in place (host -> device copies; call it outside graph capture).  The following `append` calls of
        every layer take exactly sum(counts) tokens, sequence by sequence.  A sequence whose partly filled last page is shared gets
        its own copy first (the module docstring, "Sharing")."""
        self._host("extend")
        new = [int(new_tokens_per_seq)] * self.batch if isinstance(new_tokens_per_seq, int) else [int(n) for n in new_tokens_per_seq]
        if len(new) != self.batch or min(new) < 0:
            raise ValueError(f"need {self.batch} non-negative token counts")
        need = [-(-(self.seq_lens[b] + n) // self.page_size) - len(self._pages[b]) for b, n in enumerate(new)]
        # pages wholly below the lowest position the announced tokens attend (n = 0: a decode query at the last position)
        drop = [max(self._released[b], min((self.seq_lens[b] + n - max(n, 1) - self.window + 1) // self.page_size, len(self._pages[b])))
                if self.release else 0 for b, n in enumerate(new)]
        # a dry run of the counts, in the order of the real one below: a released page is gained only when its last owner lets go,
        # and of the sequences that share a partly filled last page all but the last to be served need a copy (and a page for it)
        less, freed, cow = {}, 0, []
        for b in range(self.batch):
            for p in self._pages[b][self._released[b]:drop[b]]:
                less[p] = less.get(p, 0) + 1
                freed += self._ref[p] == less[p]
        for b, n in enumerate(new):
            if n and self.seq_lens[b] % self.page_size:
                p = self._pages[b][-1]
                if self._ref[p] - less.get(p, 0) > 1:
                    less[p] = less.get(p, 0) + 1
                    cow.append(b)
        if sum(need) + len(cow) > len(self._free) + freed:
            raise RuntimeError(f"out of pages: {sum(need) + len(cow)} needed, {len(self._free) + freed} free")
        for b in range(self.batch):                              # releases first: another sequence's new tokens may take these pages
            for i in range(self._released[b], drop[b]):
                self._unref(self._pages[b][i])
                self._pages[b][i] = -1
            self._released[b] = drop[b]
        pairs = []
        for b, n in enumerate(new):
            if b in cow:                                         # the sole-owner rule: its own copy of the rows it holds there
                old, self._pages[b][-1] = self._pages[b][-1], self._take()
                self._unref(old)
                pairs.append((old, self._pages[b][-1], self.seq_lens[b] % self.page_size))
            self._pages[b] += [self._take() for _ in range(need[b])]
            self.seq_lens[b] += n
        self._upload(new)
        self._announced = (new, [self.seq_lens[b] - n for b, n in enumerate(new)])
        if pairs:
            self._copy_pages(pairs)

    def _shorten(self, seq, length):
        """keep the first `length` tokens of `seq`: the pages wholly past them lose a reference"""
        keep = -(-length // self.page_size)
        for p in reversed(self._pages[seq][keep:]):
            if p >= 0:                                           # a released entry's reference is gone already
                self._unref(p)
        del self._pages[seq][keep:]
        self._released[seq] = min(self._released[seq], keep)
        self.seq_lens[seq] = length

    def _check_length(self, seq, length, what):
        if not 0 <= length <= self.seq_lens[seq]:
            raise ValueError(f"{what}: length {length} outside [0, {self.seq_lens[seq]}], the tokens sequence {seq} holds")
        kept = min(self._released[seq], -(-length // self.page_size))
        if kept * self.page_size > max(0, length - self.window):
            raise ValueError(f"{what}: the first {kept} pages of sequence {seq} were released below its window; {length} tokens with a "
                             f"window of {self.window} would attend tokens on them")

    def fork(self, src, dst, length=None):
        """Sequence `dst` becomes a copy of the first `length` tokens of `src` (default: all) without copying anything: `dst` is reset,
        then lists the same pages, released entries included, and each page's count goes up.  length 0 is a reset.  ValueError for src == dst,
        a length outside [0, seq_lens[src]] and a length that would put a released page inside the window (the module docstring).
        Rewrites the page table on the device like `extend` (outside graph capture)."""
        self._host("fork")
        length = self.seq_lens[src] if length is None else int(length)
        if src == dst:
            raise ValueError("fork: src and dst are the same sequence")
        self._check_length(src, length, "fork")
        self._shorten(dst, 0)
        self._pages[dst] = self._pages[src][: -(-length // self.page_size)]
        for p in self._pages[dst]:
            if p >= 0:
                self._ref[p] += 1
        self._released[dst] = min(self._released[src], len(self._pages[dst]))
        self.seq_lens[dst] = length
        self._upload([0] * self.batch)

    def truncate(self, seq, length):
        """Drop the tokens of `seq` at and past `length` (the rejected part of a speculative draft).  Nothing is copied; pages wholly
        past `length` lose a reference.  ValueError as for `fork`.  Outside graph capture."""
        self._host("truncate")
        length = int(length)
        self._check_length(seq, length, "truncate")
        self._shorten(seq, length)
        self._upload([0] * self.batch)

    def reset(self, seq):
        """Empty sequence `seq`: its pages lose a reference, and those it owned alone return to the free list (outside graph capture)."""
        self._host("reset")
        self._shorten(seq, 0)
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

    def attend(self, layer, q, max_seq_len=None, sm_scale=None, *, shared=False, max_shared_len=None):
        """Decode attention of q (bf16 [B, Hq, 128]) over `layer`.  max_seq_len defaults to the longest sequence now (host
        bookkeeping, no device sync); under graph capture pass the bound the replays will stay within.
        shared=True: the same attention through `mixedgemm.paged_decode_shared` over the groups of `share_groups()` (the module
        docstring, "Shared-prefix decode"), always, whether or not anything is shared.  Its two bounds default to host bookkeeping, the
        largest shared count and the longest tail now; under capture pass max_seq_len, which then bounds the tails, and max_shared_len."""
        if shared:
            if self.window:
                raise ValueError("attend(shared=True) has no sliding-window form: this cache was made with window="
                                 f"{self.window}; use attend()")
            if max_shared_len is None or max_seq_len is None:
                self._host("attend(shared=True) without max_seq_len and max_shared_len")
            most = self._max_shared if max_shared_len is None else int(max_shared_len)
            tail = self._max_suffix if max_seq_len is None else int(max_seq_len)
            need = mixedgemm.paged_decode_shared_workspace_bytes(self.batch, q.size(1), self.num_kv_heads, most, tail)
            if need and (self._shared_workspace is None or self._shared_workspace.numel() < need):
                if self._shared_workspace is not None:
                    self._retired.append(self._shared_workspace)      # a graph captured earlier may still point at it
                self._shared_workspace = torch.empty((need,), dtype=torch.uint8, device=self.device)
            return mixedgemm.paged_decode_shared(q, self.kv_data, self.kv_param, self.kv_indptr, self.kv_indices, self.last_page_len, layer,
                                                 self.group_indptr, self.group_members, self.shared_len, most, tail, sm_scale=sm_scale,
                                                 workspace=self._shared_workspace if need else None)
        if max_seq_len is None:
            self._host("attend without max_seq_len")
        bound = max(self.seq_lens) if max_seq_len is None else int(max_seq_len)
        need = mixedgemm.paged_decode_workspace_bytes(self.batch, q.size(1), self.num_kv_heads, bound, self.window)
        if need and (self._workspace is None or self._workspace.numel() < need):
            if self._workspace is not None:
                self._retired.append(self._workspace)      # a graph captured earlier may still point at it
            self._workspace = torch.empty((need,), dtype=torch.uint8, device=self.device)
        return mixedgemm.paged_decode(q, self.kv_data, self.kv_param, self.kv_indptr, self.kv_indices, self.last_page_len, layer, bound,
                                      sm_scale=sm_scale, workspace=self._workspace if need else None, window=self.window)

    def tree_mask(self, parents):
        """(mask, depths) of the tokens the last `extend` announced, taken as tree drafts (host work and one upload; a CPU cache works).
        parents[b]: a list of n_b ints, entry i the parent of new token i of sequence b: -1, a child of the last committed token, or the
        index of an earlier new token; or None, a causal chain.  mask: int64 [num_new_tokens] on the cache's device for
        `attend_new(tree=)`, bit i of word j set when i is j or an ancestor of j.  depths[b][i]: the nodes between i and the committed
        tokens, so node i stands at position base_b + depths[b][i], which is the cos / sin row to give `append_rope` for it.
        ValueError for a parent >= its index or < -1, a list of the wrong length, a tree of more than 64 nodes, and tables changed
        since the `extend`.  The parents are kept for `accept`, and a copy of the words for `verify_launch`: in a tensor of the cache's
        own that keeps its address while the token count does not grow, so a captured `verify_launch` replays with the next tree."""
        if self._announced is None:
            raise ValueError("tree_mask: the page tables changed since the last extend (fork, truncate, reset, accept): nothing is announced")
        counts = self._announced[0]
        if len(parents) != self.batch:
            raise ValueError(f"tree_mask: need {self.batch} parent lists (None for a chain)")
        words, depths, kept = [], [], []
        for b, (n, par) in enumerate(zip(counts, parents)):
            if par is None:
                words += [(2 << min(j, 63)) - 1 & (1 << 64) - 1 for j in range(n)]     # past 64 tokens the kernel reads no words
                depths.append(list(range(n)))
                kept.append(None)
                continue
            par = [int(p) for p in par]
            if len(par) != n:
                raise ValueError(f"tree_mask: sequence {b} announced {n} tokens, got {len(par)} parents")
            if n > 64:
                raise ValueError(f"tree_mask: a tree holds at most 64 nodes (one mask word), sequence {b} has {n}; pass None for a chain")
            w, d = [], []
            for i, p in enumerate(par):
                if not -1 <= p < i:
                    raise ValueError(f"tree_mask: parent {p} of token {i} of sequence {b} is neither -1 nor an earlier token")
                w.append((w[p] if p >= 0 else 0) | 1 << i)
                d.append(d[p] + 1 if p >= 0 else 0)
            words += w
            depths.append(d)
            kept.append(par)
        self._parents = kept
        mask = torch.tensor([x - (1 << 64) if x >> 63 else x for x in words], dtype=torch.int64).to(self.device)
        if self._tree_words is None or self._tree_words.numel() < mask.numel():
            if self._tree_words is not None:
                self._retired.append(self._tree_words)           # a graph captured earlier may still point at it
            self._tree_words = torch.zeros((max(mask.numel(), 64 * self.batch),), dtype=torch.int64, device=self.device)
        self._tree_words[: mask.numel()].copy_(mask)
        self._tree_words_live = True
        return mask, depths

    def accept(self, paths):
        """Keep one root-to-leaf path of each sequence's draft: paths[b] lists the accepted new-token indices of sequence b in ascending
        order, possibly none ([]: the whole draft is dropped); None stands for [] where nothing was announced.  The rows at positions
        base_b + paths[b][i] move to base_b + i in every layer (one `mixedgemm.kv_move_rows` launch on the current stream; on a CPU
        cache, slice assignment), sequence b is shortened to base_b + len(paths[b]) as `truncate` does, and the tables are uploaded once.
        Call it after every layer's `append`, outside graph capture.  A sequence that took its own copy of a shared last page at the
        `extend` keeps it, also when its whole draft is dropped.  ValueError when the tables changed since the `extend`, and for a
        path that is not a chain from the root under the parents of the last `tree_mask` (without one: causal chains, so a prefix
        0, 1, .. k - 1).  `verify` picks the paths on the device and does all of this without the host in between (the module
        docstring, "Verifying a draft")."""
        self._host("accept")
        checked = self._checked_paths(paths, "accept")
        bases = self._announced[1]
        indptr, src, dst = [0], [], []
        for b, path in enumerate(checked):
            for i, p in enumerate(path):
                if p != i:
                    src.append(bases[b] + p)
                    dst.append(bases[b] + i)
            indptr.append(len(src))
        if src:
            self._move_rows(indptr, src, dst)
        self._keep_paths(checked)

    def _checked_paths(self, paths, what):
        """`paths` as lists of ints, each a chain from the root of what the last `extend` announced; ValueError otherwise"""
        if self._announced is None:
            raise ValueError(f"{what}: the page tables changed since the last extend (fork, truncate, reset, accept): nothing to accept")
        counts, bases = self._announced
        if len(paths) != self.batch:
            raise ValueError(f"{what}: need {self.batch} paths")
        parents = self._parents or [None] * self.batch
        checked = []
        for b, path in enumerate(paths):
            if path is None:
                if counts[b]:
                    raise ValueError(f"{what}: sequence {b} announced {counts[b]} tokens and has no path ([] drops them all)")
                path = []
            path = [int(p) for p in path]
            for i, p in enumerate(path):
                if not 0 <= p < counts[b]:
                    raise ValueError(f"{what}: token {p} is not one of the {counts[b]} sequence {b} announced")
                parent = p - 1 if parents[b] is None else parents[b][p]
                if parent != (path[i - 1] if i else -1):
                    raise ValueError(f"{what}: token {p} of sequence {b} does not continue the path (its parent is {parent})")
            self._check_length(b, bases[b] + len(path), what)
            checked.append(path)
        return checked

    def _keep_paths(self, checked):
        """the bookkeeping after the rows of the checked paths were packed down: every sequence ends behind its path, one upload"""
        bases = self._announced[1]
        for b, path in enumerate(checked):
            self._shorten(b, bases[b] + len(path))
        self._upload([0] * self.batch)

    def verify_launch(self, target_tok, draft_tok, root_tok):
        """The device half of `verify`: `mixedgemm.verify_greedy` over the tokens the last `extend` announced -- with the cache's own
        tables, `append_indptr`, and the words of the last `tree_mask` call (chains when it was not called since the `extend`) --
        and then, on the same stream with nothing in between, `mixedgemm.kv_move_rows` from the move table it wrote.  target_tok,
        draft_tok: int32 [num_new_tokens], root_tok: int32 [batch], on the cache's device (what they mean: `mixedgemm.verify_greedy`).
        target_tok comes from `mixedgemm.argmax_rows` (greedy decoding) or `mixedgemm.sample_rows` (temperature, top-k, top-p, min-p:
        the kept path and the bonus token are then distributed as the target model's), either captured in front of this call.
        Returns the result tensor, int32 [batch, 66], the same tensor at every call; give it to `commit`.  Nothing is allocated after
        the first call with a token count, and nothing is read on the host: capturable, after every layer's `append`.  A graph
        captured with a tree replays with a tree (`tree_mask` writes the next one where the graph reads it), one captured with
        chains with chains.  ValueError on a cache made with window= when `tree_mask` was given a tree: chains only there."""
        if self.device.type == "cpu":
            raise RuntimeError("verify_launch needs a device cache; a CPU cache verifies with verify()")
        if self.window and any(p is not None for p in self._parents or ()):
            raise ValueError(f"verify_launch has no sliding-window form for trees: this cache was made with window={self.window}")
        T = self.num_new_tokens
        if self._verify_moves is None or self._verify_moves.size(1) < T:
            if self._verify_moves is not None:
                self._retired.append(self._verify_moves)         # a graph captured earlier may still point at it
            self._verify_moves = torch.full((2, max(T, 64 * self.batch)), -1, dtype=torch.int32, device=self.device)
        src, dst = self._verify_moves[0, :T], self._verify_moves[1, :T]
        mixedgemm.verify_greedy(target_tok, draft_tok, root_tok, self.append_indptr, self.kv_indptr, self.last_page_len, self.page_size,
                                tree_mask=self._tree_words[:T] if self._tree_words_live else None, result=self._verify_result,
                                move_src=src, move_dst=dst)
        mixedgemm.kv_move_rows(self.kv_data, self.kv_param, self.kv_indptr, self.kv_indices, self.append_indptr, src, dst)
        return self._verify_result

    @staticmethod
    def _paths_of(rows, counts):
        """(paths, next_tokens) from the rows of a verify result: k path entries, or -- a sequence that keeps all -- every token"""
        paths, nxt = [], []
        for row, n in zip(rows, counts):
            k = row[0]
            paths.append(list(range(k)) if k and row[2] < 0 else row[2:2 + k])
            if not n and not k:
                paths[-1] = None
            nxt.append(row[1])
        return paths, nxt

    def commit(self, result):
        """The host half of `verify`: one device-to-host copy of `result` (what `verify_launch` returned, also after a graph replay),
        then the validation and the bookkeeping of `accept` for the paths it holds -- no move is launched: the rows were packed by
        `verify_launch`.  Returns (paths, next_tokens): paths[b] as `accept` takes it (every announced token for a sequence that kept
        all, None where nothing was announced), next_tokens[b] the bonus token (`mixedgemm.verify_greedy`, result[b][1]).
        ValueError as `accept` raises it, here AFTER the rows have moved -- a path the parents of `tree_mask` do not allow, which
        includes a tree sequence that kept all (root_tok < 0): the rows of the announced tokens are then undefined, the committed
        tokens are untouched, and `truncate(b, base_b)` for every sequence (base_b = seq_lens[b] minus what it announced) recovers."""
        self._host("commit")
        if self._announced is None:
            raise ValueError("commit: the page tables changed since the last extend (fork, truncate, reset, accept): nothing to accept")
        paths, nxt = self._paths_of(result.cpu().tolist(), self._announced[0])
        self._keep_paths(self._checked_paths(paths, "commit"))
        return paths, nxt

    def verify(self, target_tok, draft_tok, root_tok):
        """Greedy verification of the tokens the last `extend` announced, after every layer's `append`: `verify_launch` then `commit`
        (the module docstring, "Verifying a draft"); returns (paths, next_tokens).  On a CPU cache the walk runs here, in plain
        Python, and `accept` moves the rows: the rule in words."""
        if self.device.type != "cpu":
            return self.commit(self.verify_launch(target_tok, draft_tok, root_tok))
        if self._announced is None:
            raise ValueError("verify: the page tables changed since the last extend (fork, truncate, reset, accept): nothing to accept")
        counts = self._announced[0]
        parents = self._parents or [None] * self.batch
        target, draft, roots = (t.tolist() for t in (target_tok, draft_tok, root_tok))
        if len(target) != self.num_new_tokens or len(draft) != self.num_new_tokens or len(roots) != self.batch:
            raise RuntimeError(f"verify expects the {self.num_new_tokens} tokens announced by extend() and {self.batch} root tokens")
        paths, nxt, q0 = [], [], 0
        for b, n in enumerate(counts):
            if n > 64 or roots[b] < 0:                           # no draft: a prompt chunk keeps all
                paths.append(list(range(n)) if n else None)
                nxt.append(target[q0 + n - 1] if n else -1)
            else:
                cur, want, path = -1, roots[b], []
                while True:
                    step = [i for i in range(n) if (i - 1 if parents[b] is None else parents[b][i]) == cur and draft[q0 + i] == want]
                    if not step:
                        break
                    cur = step[0]
                    path.append(cur)
                    want = target[q0 + cur]
                paths.append(path if n else None)
                nxt.append(want)
            q0 += n
        self.accept(paths)
        return paths, nxt

    def _move_rows(self, indptr, src, dst):
        """positions src -> dst within each sequence (indptr splits them), every layer: one launch on the current stream"""
        if self.device.type == "cpu":                            # the host tests' path, and the move rule in plain words
            P = self.page_size
            for b in range(self.batch):
                moves = range(indptr[b], indptr[b + 1])
                at = lambda pos: (self._pages[b][pos // P], slice(None), slice(None), slice(None), pos % P)
                rows = [(self.kv_data[at(src[m])].clone(), None if self.kv_param is None else self.kv_param[at(src[m])].clone()) for m in moves]
                for m, (data, param) in zip(moves, rows):        # every source was read before the first write
                    self.kv_data[at(dst[m])] = data
                    if param is not None:
                        self.kv_param[at(dst[m])] = param
            return
        table = torch.tensor(indptr + src + dst, dtype=torch.int32).to(self.device)
        mixedgemm.kv_move_rows(self.kv_data, self.kv_param, self.kv_indptr, self.kv_indices, *table.split([len(indptr), len(src), len(dst)]))

    def attend_new(self, layer, q, max_seq_len=None, sm_scale=None, *, tree=None):
        """Causal attention of the tokens the last `extend()` announced: q (bf16 [num_new_tokens, Hq, 128], sequence by sequence) over
        `layer`, each new token attending its sequence's cache up to and including itself.  Call it after `append` of the same layer.
        max_seq_len as in `attend`.
        tree: the mask `tree_mask()` returned (int64 [num_new_tokens]): the new tokens are tree drafts, and a token attends the
        committed tokens, its ancestors among the new ones and itself (the module docstring, "Tree drafts").  ValueError on a cache
        made with window=."""
        if tree is not None and self.window:
            raise ValueError(f"attend_new(tree=) has no sliding-window form: this cache was made with window={self.window}")
        if q.dim() != 3 or q.size(0) != self.num_new_tokens:
            raise RuntimeError(f"attend_new expects the {self.num_new_tokens} tokens announced by extend(), got q of shape {tuple(q.shape)}")
        if max_seq_len is None:
            self._host("attend_new without max_seq_len")
        bound = max(self.seq_lens) if max_seq_len is None else int(max_seq_len)
        need = mixedgemm.paged_prefill_workspace_bytes(self.num_new_tokens, self.batch, q.size(1), self.num_kv_heads, bound, self.window)
        if need and (self._prefill_workspace is None or self._prefill_workspace.numel() < need):
            if self._prefill_workspace is not None:
                self._retired.append(self._prefill_workspace)      # a graph captured earlier may still point at it
            self._prefill_workspace = torch.empty((need,), dtype=torch.uint8, device=self.device)
        return mixedgemm.paged_prefill(q, self.kv_data, self.kv_param, self.kv_indptr, self.kv_indices, self.last_page_len,
                                       self.append_indptr, layer, bound, sm_scale=sm_scale,
                                       workspace=self._prefill_workspace if need else None, window=self.window, tree_mask=tree)

    # ---- device steps ---------------------------------------------------------------------------------------------------------------------
    def _step_args(self, next_counts, max_seq_len):
        counts = [int(next_counts)] * self.batch if isinstance(next_counts, int) else [int(n) for n in next_counts]
        if len(counts) != self.batch or min(counts) < 0:
            raise ValueError(f"need {self.batch} non-negative token counts")
        max_seq_len = int(max_seq_len)
        if max_seq_len < 1:
            raise ValueError("max_seq_len must be positive")
        return counts, max_seq_len, -(-max_seq_len // self.page_size)

    def _flat_depths(self, depths, counts):
        """depths as `tree_mask` returns them (a list per sequence, None: a chain) or one flat list, as one flat list"""
        if depths is None:
            return None
        if len(depths) == self.batch and all(d is None or isinstance(d, (list, tuple)) for d in depths):
            depths = [x for d, n in zip(depths, counts) for x in (range(n) if d is None else d)]
        flat = [int(x) for x in depths]
        if len(flat) != sum(counts) or (flat and min(flat) < 0):
            raise ValueError(f"depths: need one non-negative depth for each of the {sum(counts)} announced tokens")
        return flat

    def steps_guaranteed(self, next_counts, max_seq_len):
        """How many `step_launch(result, next_counts, max_seq_len=max_seq_len)` calls in a row cannot fail, whatever the drafts keep
        (host only).  The worst case keeps every announced token, since a step that keeps less holds fewer pages and shorter
        sequences: step s then needs seq_lens[b] + s * n_b <= max_seq_len for every sequence, sum_b ceil((seq_lens[b] + s * n_b) / P)
        - (pages held now) <= the free pages, and that sum of list entries <= kv_indices.numel().  Exact for that case: this many
        steps with everything kept succeed and the next one fails.  With no token announced at all every step succeeds: 2^31 - 1."""
        self._host("steps_guaranteed")
        counts, max_seq_len, _ = self._step_args(next_counts, max_seq_len)
        if max(self._seq_lens) > max_seq_len:
            return 0
        if not any(counts):
            return (1 << 31) - 1
        held, free, P = sum(map(len, self._pages)), len(self._free), self.page_size

        def fits(s):                                             # monotone in s: entries only grow
            entries = sum(-(-(n + s * c) // P) for n, c in zip(self._seq_lens, counts))
            return entries - held <= free and entries <= self.kv_indices.numel()

        lo, hi = 0, min((max_seq_len - n) // c for n, c in zip(self._seq_lens, counts) if c)    # by length; then bisect on the pages
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if fits(mid) else (lo, mid - 1)
        return lo

    def _check_sole_owner(self, what):
        for b, n in enumerate(self._seq_lens):
            if n % self.page_size and self._ref[self._pages[b][-1]] > 1:
                raise ValueError(f"{what}: sequence {b} shares its partly filled last page; a host extend() that announces tokens for it "
                                 "takes its own copy first")
        if any(p < 0 for pages in self._pages for p in pages):
            raise ValueError(f"{what}: pages were released below a window; device steps keep every page")

    def _pack_state(self, max_seq_len, pps):
        """the state of mixedgemm.kv_step (include/micromix_kvstep.h) from the host lists, as one list"""
        announced = self._announced[0] if self._announced is not None else [0] * self.batch
        for b, pages in enumerate(self._pages):
            if len(pages) > pps or self._seq_lens[b] > max_seq_len:
                raise ValueError(f"step_launch: sequence {b} holds {self._seq_lens[b]} tokens, more than max_seq_len = {max_seq_len}")
        flat = [0, 0, len(self._free), 0] + self._seq_lens + list(announced) + [len(p) for p in self._pages]
        flat += self._free + [0] * (self.max_pages - len(self._free))
        for pages in self._pages:
            flat += pages + [0] * (pps - len(pages))
        return flat

    def upload_state(self, max_seq_len, next_counts=None, depths=None):
        """Make the device state of `step_launch` current now (one host-to-device copy, outside capture).  With next_counts (and the
        depths `step_launch` will be given) it also uploads those and allocates token_pos: everything `step_launch(result, next_counts,
        max_seq_len=max_seq_len, depths=depths)` would do outside capture, so that the FIRST such call can already be captured.
        `step_launch` does all of this itself when it is not capturing.  Call it again before replaying a graph of steps whenever
        host calls (extend, fork, truncate, ...) changed the tables since: the graph reads the state that was uploaded last."""
        self._host("upload_state")
        if self.release:
            raise ValueError("device steps do not release pages below a window: this cache was made with window= and release on")
        counts, max_seq_len, pps = self._step_args(0 if next_counts is None else next_counts, max_seq_len)
        self._check_sole_owner("upload_state")
        flat = self._pack_state(max_seq_len, pps)
        if self.device.type == "cpu":
            return
        if self._step_state is None or self._step_state.numel() != len(flat):
            if self._step_state is not None:
                self._retired.append(self._step_state)          # a graph captured earlier may still point at it
            self._step_state = torch.zeros((len(flat),), dtype=torch.int32, device=self.device)
        self._step_state.copy_(torch.tensor(flat, dtype=torch.int32))
        self._step_geometry = (max_seq_len, pps)
        self._state_current = True
        self._steps_seen = 0
        if next_counts is not None:
            self._step_buffers(counts, depths, False)

    @property
    def step_state(self):
        """the device state of `step_launch` (include/micromix_kvstep.h), or None before the first upload: what `mixedgemm.token_step`
        takes as kv_state, so that the token history stops where the page table did.  The same tensor until the geometry changes"""
        return self._step_state

    def _step_buffers(self, counts, depths, capturing):
        """next_counts, depths and token_pos where the kernel reads and writes them; returns the depths tensor or None.  Uploads and
        allocations happen only when something differs from the last call, and raise under capture"""
        T = sum(counts)
        if counts != self._step_counts:
            if capturing:
                raise RuntimeError("step_launch under stream capture with new next_counts: they are uploaded outside capture")
            if self._next_new is None:
                self._next_new = torch.zeros((self.batch,), dtype=torch.int32, device=self.device)
            self._next_new.copy_(torch.tensor(counts, dtype=torch.int32))
            self._step_counts = counts
        if self._token_pos is None or self._token_pos.numel() < T:
            if capturing:
                raise RuntimeError("step_launch under stream capture would allocate token_pos: call it once outside capture")
            if self._token_pos is not None:
                self._retired.append(self._token_pos)
            self._token_pos = torch.zeros((max(T, 64 * self.batch),), dtype=torch.int32, device=self.device)
            self._token_pos_view = None
        if self._token_pos_view is None or self._token_pos_view.numel() != T:
            self._token_pos_view = self._token_pos[:T]
        if isinstance(depths, torch.Tensor):
            return depths
        flat = self._flat_depths(depths, counts)
        if flat is not None and (flat != self._step_depths or self._depths_dev is None or self._depths_dev.numel() < T):
            if capturing:
                raise RuntimeError("step_launch under stream capture with new depths: they are uploaded outside capture")
            if self._depths_dev is None or self._depths_dev.numel() < T:
                if self._depths_dev is not None:
                    self._retired.append(self._depths_dev)
                self._depths_dev = torch.zeros((max(T, 64 * self.batch),), dtype=torch.int32, device=self.device)
            self._depths_dev[:T].copy_(torch.tensor(flat, dtype=torch.int32))
            self._step_depths = flat
        return None if flat is None or not T else self._depths_dev[:T]

    def step_launch(self, result, next_counts, *, max_seq_len, depths=None):
        """Commit the announced tokens and announce the next ones ON THE DEVICE: what `commit(result)` + `extend(next_counts)` do, without
        the host (the module docstring, "Device steps"; the rule: include/micromix_kvstep.h).  Returns token_pos, int32 [T], T =
        sum(next_counts): the position of every new token, its cos / sin row for `append_rope`; the same tensor at every call.
        result: what `verify_launch` returned (its column 0 is the number of announced tokens each sequence keeps, already packed down by
        its moves), or None: every announced token stays, the plain decode loop.  next_counts: an int or one host int per sequence.
        depths: the depths of the new tokens as `tree_mask` returns them, a flat list, or an int32 device tensor [T] of the caller's
        that the kernel reads at every replay; None: chains.  max_seq_len: no sequence may grow past it; it sizes the state
        (ceil(max_seq_len / P) list entries per sequence) and has to stay the same while the device is ahead.
        Capturable once the device state is current: the counts and depths are uploaded only when they differ from the last call's, the
        state only when the host tables changed since it was uploaded (any extend, fork, truncate, reset, accept) -- under stream capture
        either raises RuntimeError; `upload_state(max_seq_len, next_counts, depths)` or one call outside capture prepares all of it.  Nothing is read on the host: a
        step that cannot be taken (no page left, a sequence past max_seq_len, ...) leaves every table as it was and sets a sticky
        status that `sync()` raises; `steps_guaranteed` says how many steps cannot fail.
        On entry with the host current, no sequence's partly filled last page may be shared (ValueError; the host `extend` that announced
        its tokens made it so).  Device steps keep that: after a step a sequence's last page is the page it wrote before, still its own,
        or a page popped from the free stack, which no list names; pages below the announced tokens are never touched.
        ValueError on a cache whose window releases pages: eviction stays on the host.  The announced counts become next_counts, so
        `tree_mask` (outside capture) and `verify_launch` work for the next step; when next_counts equal the counts announced before,
        the tree of the last `tree_mask` call stays in force: a fixed topology needs no call between the steps.
        On a CPU cache the rule runs here in plain Python over the lists, and a step that cannot be taken raises RuntimeError at once."""
        if self.release:
            raise ValueError("step_launch does not release pages below a window: this cache was made with window= and release on")
        counts, max_seq_len, pps = self._step_args(next_counts, max_seq_len)
        T = sum(counts)
        if result is not None and self._announced is None:
            raise ValueError("step_launch: the page tables changed since the last extend (fork, truncate, reset, accept): nothing to keep")
        same = self._announced is not None and list(self._announced[0]) == counts
        tree = (self._parents, self._tree_words_live) if same else (None, False)
        if self.device.type == "cpu":
            token_pos = self._step_host(result, counts, max_seq_len, pps, self._flat_depths(depths, counts))
            self._parents, self._tree_words_live = tree
            return token_pos
        capturing = torch.cuda.is_current_stream_capturing()
        if self._ahead and self._step_geometry != (max_seq_len, pps):
            raise RuntimeError(f"step_launch: max_seq_len was {self._step_geometry[0]} when the device went ahead; call sync() before changing it")
        if not self._ahead and not (self._state_current and self._step_geometry == (max_seq_len, pps)):
            if capturing:
                raise RuntimeError("step_launch under stream capture with a stale device state: the host tables changed since it was "
                                   "uploaded; call upload_state(max_seq_len, next_counts, depths), or step_launch once, outside capture")
            self.upload_state(max_seq_len)
        depths_dev = self._step_buffers(counts, depths, capturing)
        mixedgemm.kv_step(self._step_state, self.max_pages, pps, self.page_size, max_seq_len, self._next_new, T, self.kv_indptr, self.kv_indices,
                          self.last_page_len, self.append_indptr, keep=result, depths=depths_dev, token_pos=self._token_pos_view if T else None)
        self._ahead = True
        self._captured |= capturing
        self.num_new_tokens = T
        self._announced = (counts, None)                        # the bases are the device's until sync()
        self._parents, self._tree_words_live = tree
        return self._token_pos_view

    def _step_host(self, result, counts, max_seq_len, pps, depths):
        """the rule of include/micromix_kvstep.h in plain words, on a CPU cache's own lists"""
        P, status = self.page_size, _lib.KV_STEP
        announced = list(self._announced[0]) if self._announced is not None else [0] * self.batch
        if result is None:
            keep = announced
        else:
            keep = [int(k) for k in (result[:, 0] if isinstance(result, torch.Tensor) and result.dim() == 2 else result)]
        self._check_sole_owner("step_launch")
        self._pack_state(max_seq_len, pps)                       # its refusals
        kept = [n - a + k for n, a, k in zip(self._seq_lens, announced, keep)]
        final = [n + c for n, c in zip(kept, counts)]
        keep_pages, final_pages = [-(-n // P) for n in kept], [-(-n // P) for n in final]
        pushes = sum(len(pages) - kp for pages, kp in zip(self._pages, keep_pages))
        failed = None
        if any(not 0 <= k <= a for k, a in zip(keep, announced)):
            failed = "MM_KV_STEP_BAD_KEEP"
        elif max(final) > max_seq_len:
            failed = "MM_KV_STEP_TOO_LONG"
        elif sum(final_pages) - sum(keep_pages) > len(self._free) + pushes:
            failed = "MM_KV_STEP_OUT_OF_PAGES"
        elif sum(final_pages) > self.kv_indices.numel():
            failed = "MM_KV_STEP_INDICES_CAPACITY"
        if failed:
            raise RuntimeError(f"step_launch: the step cannot be taken: {failed} ({status[failed]}); nothing was changed")
        for b in range(self.batch):                              # 1: shorten; the pages past the kept tokens go back, highest entry first
            for p in reversed(self._pages[b][keep_pages[b]:]):
                self._unref(p)
            del self._pages[b][keep_pages[b]:]
        for b in range(self.batch):                              # 2: after all are shortened, the new tokens' pages in pop order
            self._pages[b] += [self._take() for _ in range(final_pages[b] - keep_pages[b])]
            self._seq_lens[b] = final[b]
        self._upload(counts)                                     # 3: the tables
        self._announced = (counts, kept)
        pos = [kept[b] + i for b, n in enumerate(counts) for i in range(n)] if depths is None else \
              [kept[b] + d for b, n in enumerate(counts) for d in depths[sum(counts[:b]):sum(counts[:b]) + n]]
        return torch.tensor(pos, dtype=torch.int32)

    def sync(self):
        """Bring the host lists up to the device: one device-to-host copy of the state, from which `_pages`, the free list (in the
        stack's order), the reference counts (recounted from the lists) and `seq_lens` are rebuilt; the tokens of the last announce
        are announced again on the host, so `commit` / `accept` can close the last step, and `extend` etc. work again.  The
        copy is made whenever a state is on the device that the host has not replaced since -- also when no `step_launch` ran in
        Python, because a replayed graph moves the device without it -- and the lists are rebuilt when the state's step count or
        status says that steps were taken.  Call it after the replays whose result the host wants.  RuntimeError when a step failed, naming its number (from 0, counted from the last upload
        of the state) and its status; the host state is then that of the last good step, which is also what the device tables hold,
        and the next `step_launch` uploads the state again."""
        if self._step_state is None or not self._state_current:
            return                                               # the host lists are the newer ones
        flat = self._step_state.cpu().tolist()
        B, H = self.batch, _lib.KV_STEP["MM_KV_STEP_HEADER_INTS"]
        status, steps_done, free_count, failed_step = flat[:H]
        if not self._ahead and not status and steps_done == self._steps_seen:
            return                                               # nothing ran since the host last looked
        self._steps_seen = steps_done
        pps = self._step_geometry[1]
        lens, announced, num_pages = flat[H:H + B], flat[H + B:H + 2 * B], flat[H + 2 * B:H + 3 * B]
        stack = flat[H + 3 * B:H + 3 * B + self.max_pages]
        lists = H + 3 * B + self.max_pages
        self._pages = [flat[lists + b * pps:lists + b * pps + num_pages[b]] for b in range(B)]
        self._free = stack[:free_count]
        self._ref = [0] * self.max_pages
        for pages in self._pages:
            for p in pages:
                self._ref[p] += 1
        assert all((self._ref[p] == 0) == (n == 1) for p, n in enumerate(self._count_free())), "a page is both listed and free, or neither"
        self._seq_lens = lens
        self._ahead = False
        self._announced = (announced, [n - a for n, a in zip(lens, announced)])
        self.num_new_tokens = sum(announced)
        self._max_suffix = max(n - c for n, c in zip(lens, self._shared_host))
        if status:
            self._state_current = False
            raise RuntimeError(f"sync: device step {failed_step} could not be taken: {_lib.KV_STEP_STATUS.get(status, status)} ({status}); "
                               "the tables and the host state are those of the last good step")

    def _count_free(self):
        seen = [0] * self.max_pages
        for p in self._free:
            seen[p] += 1
        return seen
