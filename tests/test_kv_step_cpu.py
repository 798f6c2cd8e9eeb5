"""CPU tests of the device steps of the paged KV cache: the host side of mm_kv_step (include/micromix_kvstep.h: the symbols, the
prototype, every status of the call without device work, the size function), PagedKVCache.step_launch on CPU-device caches -- the rule
in plain Python -- next to a twin cache that runs today's accept + extend and next to tests/kv_step_oracle.py, and steps_guaranteed.
No kernel is launched here."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from micromix_amd import _lib, mixedgemm
from micromix_amd.kvcache import PagedKVCache
import kv_step_oracle as ko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD, UNS = _lib.MM_OK, _lib.MM_ERR_BAD_ARG, _lib.MM_ERR_UNSUPPORTED


def cpu_cache(P, max_pages, batch, **kw):
    return PagedKVCache(num_layers=2, num_kv_heads=1, page_size=P, max_pages=max_pages, batch=batch, kind="bf16", device="cpu", **kw)


def tables(c):
    n = int(c.kv_indptr[-1])
    return c.kv_indptr.tolist(), c.kv_indices[:n].tolist(), c.last_page_len.tolist(), c.append_indptr.tolist()


def same_state(a, b):
    assert a._pages == b._pages and a._free == b._free and a._ref == b._ref and a.seq_lens == b.seq_lens
    assert tables(a) == tables(b)


# ---- the C ABI and the Python names ---------------------------------------------------------------------------------------------------
def test_symbols_prototype_and_exports():
    """fails without the feature: the header, the symbols, KVSTEP_EXPORTS and the Python names do not exist there"""
    lib = _lib.load()
    assert _lib.KVSTEP_EXPORTS == ("mm_kv_step_state_ints", "mm_kv_step")
    others = (set(_lib.EXPORTS) | set(_lib.DIAG_EXPORTS) | set(_lib.CALIB_EXPORTS) | set(_lib.LOGPROB_EXPORTS) | set(_lib.LOGITS_EXPORTS)
              | set(_lib.SPEC_EXPORTS))
    assert not set(_lib.KVSTEP_EXPORTS) & others
    assert lib.mm_version() == 660
    v, i, ll, z = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_size_t
    assert hasattr(lib, "mm_kv_step") and hasattr(lib, "mm_kv_step_state_ints")
    assert lib.mm_kv_step.restype is i and list(lib.mm_kv_step.argtypes) == [v, i, i, i, i, i, v, i, v, i, v, v, v, ll, v, v, v, v]
    assert lib.mm_kv_step_state_ints.restype is z and list(lib.mm_kv_step_state_ints.argtypes) == [i, i, i]
    # the header's integers: the oracle's, by name and value, and none of them among the MM_* attributes of _lib
    consts = _lib.constants(_lib.header_text("micromix_kvstep.h"))
    assert consts == _lib.KV_STEP and consts["MM_KV_STEP_MAX_BATCH"] == 1024 and consts["MM_KV_STEP_HEADER_INTS"] == ko.HEADER_INTS
    assert [consts[n] for n in ko.NAMES] == list(range(9)) and len(consts) == 11
    assert _lib.KV_STEP_STATUS == dict(enumerate(ko.NAMES)) and not any(hasattr(_lib, n) for n in consts)
    for name in ("kv_step", "kv_step_state_ints"):
        assert name in mixedgemm.__all__ and callable(getattr(mixedgemm, name)), name
    sig = inspect.signature(mixedgemm.kv_step).parameters
    assert list(sig) == ["state", "max_pages", "pages_per_seq", "page_size", "max_seq_len", "next_new", "num_next_tokens", "kv_indptr",
                         "kv_indices", "last_page_len", "append_indptr", "keep", "depths", "token_pos"]
    assert all(sig[n].kind is inspect.Parameter.KEYWORD_ONLY and sig[n].default is None for n in ("keep", "depths", "token_pos"))
    for name in ("step_launch", "sync", "steps_guaranteed", "upload_state"):
        assert callable(getattr(PagedKVCache, name)), name
    sig = inspect.signature(PagedKVCache.step_launch).parameters
    assert list(sig) == ["self", "result", "next_counts", "max_seq_len", "depths"]
    assert sig["max_seq_len"].kind is inspect.Parameter.KEYWORD_ONLY and sig["max_seq_len"].default is inspect.Parameter.empty
    assert isinstance(PagedKVCache.seq_lens, property)
    import importlib.util
    spec = importlib.util.spec_from_file_location("dropin_mixedgemm_kvstep", os.path.join(ROOT, "micromix_amd", "dropin", "mixedgemm.py"))
    dropin = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dropin)
    assert dropin.kv_step is mixedgemm.kv_step and dropin.kv_step_state_ints is mixedgemm.kv_step_state_ints
    # why no reference counts are needed on the device, and what the caller has to see to: said in the header
    header = open(os.path.join(ROOT, "include", "micromix_kvstep.h")).read()
    assert "never shared" in header and "No reference counts" in header and "HIGHEST ENTRY FIRST" in header


def test_statuses_without_device_work():
    """every row returns before a launch: the addresses are fakes or null"""
    lib = _lib.load()

    def step(state=16, batch=3, max_pages=10, pps=4, P=16, max_len=64, keep=32, stride=66, nxt=48, T=5, depths=64, indptr=80, indices=96,
             cap=10, last=112, app=128, pos=144):
        return lib.mm_kv_step(state, batch, max_pages, pps, P, max_len, keep, stride, nxt, T, depths, indptr, indices, cap, last, app, pos, None)

    assert step(batch=0) == OK
    assert step(batch=0, state=None, keep=None, nxt=None, depths=None, indptr=None, indices=None, last=None, app=None, pos=None) == OK
    for name in ("state", "nxt", "indptr", "indices", "last", "app"):
        assert step(**{name: None}) == BAD, name
    for name in ("batch", "max_pages", "pps", "P", "max_len"):
        assert step(**{name: -1}) == BAD, name
        if name != "batch":
            assert step(**{name: 0}) == BAD and step(batch=0, **{name: 0}) == BAD, name       # geometry is checked also for batch == 0
    assert step(T=-1) == BAD and step(cap=-1) == BAD
    assert step(stride=0) == BAD and step(stride=-66) == BAD
    assert step(depths=64, pos=None) == BAD                                                    # depths have nowhere to go
    for name in ("state", "keep", "nxt", "depths", "indptr", "indices", "last", "app", "pos"):
        for off in (1, 2, 3):
            assert step(**{name: 160 + off}) == BAD, name                                      # 4-byte entries
    assert step(batch=1025) == UNS and step(batch=1 << 20) == UNS
    assert step(batch=1025, P=0) == BAD and step(batch=1025, T=-1) == BAD                      # a refusal comes before a limit
    assert step(batch=1024, max_pages=(1 << 31) - 1, pps=1) == UNS                              # a state past 2^31 - 1 entries
    assert step(batch=1024, max_pages=10, pps=1 << 22) == UNS


def test_the_size_function():
    size = _lib.load().mm_kv_step_state_ints
    for B, M, S in ((1, 1, 1), (3, 10, 4), (64, 600, 37), (1024, 4096, 512)):
        want = ko.HEADER_INTS + 3 * B + M + B * S
        assert size(B, M, S) == want == mixedgemm.kv_step_state_ints(B, M, S) == ko.State([0] * B, [0] * B, [[]] * B, [], M, S).ints()
        assert len(ko.State([0] * B, [0] * B, [[]] * B, [], M, S).pack()) == want
    assert size(0, 10, 4) == 0 and size(-1, 10, 4) == 0 and size(3, 0, 4) == 0 and size(3, 10, 0) == 0 and size(1025, 10, 4) == 0
    assert size(1024, (1 << 31) - 1, 1) == 0 and size(1024, 10, 1 << 22) == 0


def test_python_argument_errors():
    i = lambda n: torch.zeros((n,), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mixedgemm.kv_step(i(40), 10, 4, 16, 64, i(3), 0, i(4), i(10), i(3), i(4))
    with pytest.raises(TypeError):
        mixedgemm.kv_step(None, 10, 4, 16, 64, i(3), 0, i(4), i(10), i(3), i(4))
    with pytest.raises(TypeError):
        mixedgemm.kv_step(i(40), 10, 4, 16, 64, i(3), 0, i(4), i(10), i(3), i(4), None)         # keep is keyword-only


# ---- the twin: step_launch on one CPU cache, accept(prefix paths) + extend on the other --------------------------------------------------
COUNTS = (0, 1, 5, 21, 70)


@pytest.mark.parametrize("P", [1, 16, 24])
def test_twin_caches_and_the_oracle_over_200_random_steps(P):
    rng = np.random.default_rng(100 + P)
    B, max_pages, max_len = 5, 600, 30 * P + 70
    a, t = cpu_cache(P, max_pages, B), cpu_cache(P, max_pages, B)
    first = [int(x) for x in rng.integers(0, 3 * P + 2, B)]
    a.extend(first), t.extend(first)
    same_state(a, t)
    steps = forks = cuts = it = 0
    while steps < 200:
        it += 1
        announced = a._announced[0] if a._announced is not None else [0] * B
        keep = [int(rng.integers(0, n + 1)) for n in announced]
        if it % 7 == 3:                                      # the planted edges: base + k a multiple of P, and k = 0 where base % P == 0
            keep = [min(n, (-(a.seq_lens[b] - n)) % P) for b, n in enumerate(announced)]
        nxt = [int(COUNTS[x]) for x in rng.integers(0, len(COUNTS), B)]
        if it % 11 == 5:
            nxt = [0] * B
        if it % 37 == 20:                                    # a fork, then the host extend that copies the shared last page
            a.fork(0, 1), t.fork(0, 1)
            a.extend(1), t.extend(1)
            forks += 1
            same_state(a, t)
            continue
        # keep the sequences inside the pool: the longest are cut back on both caches, and since a cut may end inside a page that a fork
        # shares, the next tokens are announced by the host extend, which takes the copy (step_launch would refuse)
        if sum(a.seq_lens) + sum(nxt) > (max_pages - 2 * B) * P or max(a.seq_lens) + max(nxt) > max_len:
            while sum(a.seq_lens) + sum(nxt) > (max_pages - 2 * B) * P or max(a.seq_lens) + max(nxt) > max_len:
                b = int(np.argmax(a.seq_lens))
                n = int(rng.integers(0, P + 2))
                a.truncate(b, n), t.truncate(b, n)
                cuts += 1
            nxt = [max(n, 1) for n in nxt]                   # every sequence: one that gets no token keeps sharing its last page
            a.extend(nxt), t.extend(nxt)
            same_state(a, t)
            continue
        st = ko.from_cache(a, max_len)
        have = a._announced is not None
        depths = None if it % 3 else [int(x) for x in rng.integers(0, 9, sum(nxt))]
        pos = a.step_launch(torch.tensor(keep, dtype=torch.int32) if have else None, nxt, max_seq_len=max_len, depths=depths)
        if have:
            t.accept([list(range(k)) if n else None for k, n in zip(keep, announced)])
        t.extend(nxt)
        same_state(a, t)
        assert a._announced == t._announced and a.num_new_tokens == t.num_new_tokens == sum(nxt)
        want = ko.step(st, P, max_len, keep if have else None, nxt, sum(nxt), a.kv_indices.numel(), depths)
        assert want is not None and st.status == 0
        assert (st.pages, st.free, st.seq_len, st.announced) == (a._pages, a._free, a.seq_lens, a._announced[0])
        assert tables(a) == want[:4] and pos.tolist() == want[4] and pos.dtype is torch.int32
        steps += 1
    assert forks >= 3 and cuts >= 1 and it < 1000, (it, forks, cuts)


def test_step_launch_refusals_on_the_host():
    with pytest.raises(ValueError, match="window"):
        cpu_cache(4, 50, 2, window=8).step_launch(None, 1, max_seq_len=64)
    assert cpu_cache(4, 50, 2, window=8, release=False).step_launch(None, 1, max_seq_len=64).tolist() == [0, 0]
    c = cpu_cache(4, 50, 2)
    c.extend([6, 0])
    c.fork(0, 1)
    with pytest.raises(ValueError, match="shares its partly filled last page"):
        c.step_launch(None, 1, max_seq_len=64)
    with pytest.raises(ValueError, match="nothing to keep"):
        c.step_launch(torch.zeros((2,), dtype=torch.int32), 1, max_seq_len=64)
    c.extend(1)                                               # the copy-on-write
    assert c.step_launch(None, 1, max_seq_len=64).tolist() == [7, 7]
    with pytest.raises(ValueError, match="max_seq_len"):
        c.step_launch(None, 1, max_seq_len=7)                 # a sequence already holds 8
    with pytest.raises(ValueError, match="token counts"):
        c.step_launch(None, [1], max_seq_len=64)
    with pytest.raises(ValueError, match="depth"):
        c.step_launch(None, 1, max_seq_len=64, depths=[0])
    before = (tables(c), [list(p) for p in c._pages], list(c._free), list(c.seq_lens))
    with pytest.raises(RuntimeError, match=r"MM_KV_STEP_BAD_KEEP \(2\)"):
        c.step_launch(torch.tensor([2, 0], dtype=torch.int32), 1, max_seq_len=64)
    assert before == (tables(c), c._pages, c._free, c.seq_lens)
    c.sync()                                                  # nothing to do: a CPU cache is never ahead


def test_a_kept_tree_stays_in_force_for_a_fixed_topology():
    c = cpu_cache(4, 50, 2)
    c.extend([3, 2])
    c.tree_mask([[-1, -1, 0], None])
    parents = c._parents
    c.step_launch(torch.tensor([1, 2], dtype=torch.int32), [3, 2], max_seq_len=64)
    assert c._parents is parents and c._tree_words_live
    c.step_launch(torch.tensor([1, 2], dtype=torch.int32), [2, 2], max_seq_len=64)
    assert c._parents is None and not c._tree_words_live


# ---- steps_guaranteed ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P, max_pages, first, counts, max_len, status", [
    (16, 40, [5, 17, 0], [1, 1, 1], 4096, ko.OUT_OF_PAGES),               # the pool runs out
    (16, 600, [5, 17, 0], [1, 2, 0], 100, ko.TOO_LONG),                    # sequence 1 reaches max_seq_len: 17 + 2 s <= 100
    (1, 30, [3, 3], [5, 21], 4096, ko.OUT_OF_PAGES),
    (24, 600, [23, 100], [21, 70], 240, ko.TOO_LONG),                      # 100 + 70 s <= 240: exactly 2
    (4, 12, [16, 16, 16], [1, 1, 1], 64, ko.OUT_OF_PAGES),                 # none at all
])
def test_steps_guaranteed_is_exact(P, max_pages, first, counts, max_len, status):
    c = cpu_cache(P, max_pages, len(first))
    c.extend(first)
    n = c.steps_guaranteed(counts, max_len)
    st = ko.from_cache(c, max_len)
    for s in range(n):
        c.step_launch(None, counts, max_seq_len=max_len)      # everything kept: the worst case
        assert ko.step(st, P, max_len, None, counts, sum(counts), c.kv_indices.numel()) is not None
        assert c.steps_guaranteed(counts, max_len) == n - s - 1
    assert c.seq_lens == [f + n * k for f, k in zip(first, counts)]
    before = (tables(c), [list(p) for p in c._pages], list(c._free))
    with pytest.raises(RuntimeError, match=ko.NAMES[status]):
        c.step_launch(None, counts, max_seq_len=max_len)
    assert before == (tables(c), c._pages, c._free)
    assert ko.step(st, P, max_len, None, counts, sum(counts), c.kv_indices.numel()) is None and st.status == status and st.failed_step == n


def test_steps_guaranteed_edges():
    c = cpu_cache(16, 40, 2)
    c.extend([5, 9])
    assert c.steps_guaranteed(0, 64) == (1 << 31) - 1 and c.steps_guaranteed([0, 0], 64) == (1 << 31) - 1
    assert c.steps_guaranteed(1, 8) == 0                      # a sequence is already past it
    assert c.steps_guaranteed([1, 0], 64) == 59
    assert c.steps_guaranteed([1, 0], 1 << 30) == 619         # by pages: 1 + ceil((5 + s) / 16) <= 40; found by bisection, not a walk
    with pytest.raises(ValueError):
        c.steps_guaranteed([1], 64)
