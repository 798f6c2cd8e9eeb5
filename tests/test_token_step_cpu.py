"""CPU tests of the token half of a decode step (include/micromix_tokens.h: mm_token_step, mm_ngram_draft,
mm_ngram_draft_workspace_bytes): the header, the symbols, the prototypes and the Python names; every status of the calls without device
work; the workspace size; mixedgemm.token_step / ngram_draft on CPU tensors -- the rule in plain Python -- against tests/token_oracle.py
on seeded small-alphabet cases; and the loop ngram_draft -> model -> verify -> token_step on CPU tensors against the plain rollout.
No kernel is launched here."""
import ctypes
import inspect
import os
import random

import pytest
import torch

from micromix_amd import _lib, mixedgemm
from micromix_amd.kvcache import PagedKVCache
import token_oracle as to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD, UNS = _lib.MM_OK, _lib.MM_ERR_BAD_ARG, _lib.MM_ERR_UNSUPPORTED
i32 = lambda x: torch.tensor(x, dtype=torch.int32)


# ---- the C ABI and the Python names ---------------------------------------------------------------------------------------------------
def test_symbols_prototypes_and_exports():
    """fails without the feature: the header, the symbols, TOKENS_EXPORTS and the Python names do not exist there"""
    lib = _lib.load()
    assert _lib.TOKENS_EXPORTS == ("mm_token_step", "mm_ngram_draft_workspace_bytes", "mm_ngram_draft")
    others = (set(_lib.EXPORTS) | set(_lib.DIAG_EXPORTS) | set(_lib.CALIB_EXPORTS) | set(_lib.LOGPROB_EXPORTS) | set(_lib.LOGITS_EXPORTS)
              | set(_lib.SPEC_EXPORTS) | set(_lib.KVSTEP_EXPORTS))
    assert not set(_lib.TOKENS_EXPORTS) & others
    assert lib.mm_version() == 660
    v, i, ll, z = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_size_t
    assert all(hasattr(lib, n) for n in _lib.TOKENS_EXPORTS)
    assert lib.mm_token_step.restype is i and list(lib.mm_token_step.argtypes) == [v, ll, i, v, v, v, i, v, i, v, v, v, v, i, v, v, v]
    assert lib.mm_ngram_draft.restype is i and list(lib.mm_ngram_draft.argtypes) == [v, ll, i, v, v, i, i, i, v, v, v, v, v, v, v, z, v]
    assert lib.mm_ngram_draft_workspace_bytes.restype is z and list(lib.mm_ngram_draft_workspace_bytes.argtypes) == [i, ll]
    consts = _lib.constants(_lib.header_text("micromix_tokens.h"))
    assert consts == _lib.TOKENS == dict(MM_NGRAM_MAX_N=16, MM_NGRAM_CHUNK=8192, MM_TOKENS_MAX_LD=1 << 24, MM_TOKENS_MAX_BATCH=65535,
                                         MM_TOKENS_MAX_STOP=64, MM_TOKENS_RUNNING=to.RUNNING, MM_TOKENS_STOPPED=to.STOPPED,
                                         MM_TOKENS_LENGTH=to.LENGTH)
    assert not any(hasattr(_lib, n) for n in consts) and _lib.MM_VERIFY_STRIDE == to.STRIDE
    for name in ("token_step", "ngram_draft", "ngram_draft_workspace_bytes"):
        assert name in mixedgemm.__all__ and callable(getattr(mixedgemm, name)), name
    sig = inspect.signature(mixedgemm.token_step).parameters
    assert list(sig) == ["tokens", "total_len", "finished", "result", "target_tok", "qo_indptr", "root_tok", "max_total", "stop_tok", "kv_state",
                         "emitted"]
    assert all(sig[n].kind is inspect.Parameter.KEYWORD_ONLY and sig[n].default is None for n in ("stop_tok", "kv_state", "emitted"))
    sig = inspect.signature(mixedgemm.ngram_draft).parameters
    assert list(sig) == ["tokens", "total_len", "next_indptr", "num_tokens", "min_n", "max_n", "draft_tok", "root_tok", "cand_tok", "match_len",
                         "row_seq", "row_total_len", "workspace"]
    assert all(sig[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig)[4:])
    assert isinstance(PagedKVCache.step_state, property)
    import importlib.util
    spec = importlib.util.spec_from_file_location("dropin_mixedgemm_tokens", os.path.join(ROOT, "micromix_amd", "dropin", "mixedgemm.py"))
    dropin = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dropin)
    assert dropin.token_step is mixedgemm.token_step and dropin.ngram_draft is mixedgemm.ngram_draft
    header = open(os.path.join(ROOT, "include", "micromix_tokens.h")).read()
    assert "THE LONGEST N-GRAM, AND AMONG EQUALS THE LATEST" in header and "THE WHOLE CALL WRITES NOTHING" in header
    assert "ONE INTEGER KEY" in header and "nothing at or past N is read" in header


def test_the_source_is_a_product_source():
    from micromix_amd import build
    assert "token_step.hip" in build.SOURCES and any(h.endswith("micromix_tokens.h") for h in build.HEADERS)
    text = open(os.path.join(build.CSRC, "token_step.hip")).read()
    assert "float" not in text and "double" not in text and "atomic" not in text.replace("no atomic", "")


def test_token_step_statuses_without_device_work():
    """every row returns before a launch: the addresses are fakes or null"""
    lib = _lib.load()

    def step(tokens=16, ld=100, batch=3, total=32, fin=48, result=64, stride=66, target=80, T=9, qo=96, root=112, most=128, stop=144,
             n_stop=2, kv=160, emitted=176):
        return lib.mm_token_step(tokens, ld, batch, total, fin, result, stride, target, T, qo, root, most, stop, n_stop, kv, emitted, None)

    assert step(batch=0) == OK
    assert step(batch=0, tokens=None, total=None, fin=None, result=None, target=None, qo=None, root=None, most=None, stop=None, n_stop=0,
                kv=None, emitted=None) == OK
    for name in ("tokens", "total", "fin", "result", "target", "qo", "root", "most"):
        assert step(**{name: None}) == BAD, name
    assert step(batch=-1) == BAD and step(ld=0) == BAD and step(ld=-5) == BAD and step(T=-1) == BAD and step(batch=0, ld=0) == BAD
    assert step(stride=65) == BAD and step(stride=1) == BAD and step(stride=0) == BAD and step(stride=-66) == BAD
    assert step(n_stop=-1) == BAD and step(stop=None) == BAD and step(n_stop=0) == BAD      # the list and its length come together
    for name in ("tokens", "total", "fin", "result", "target", "qo", "root", "most", "stop", "kv", "emitted"):
        for off in (1, 2, 3):
            assert step(**{name: 192 + off}) == BAD, name                                      # 4-byte entries
    assert step(batch=65536) == UNS and step(ld=(1 << 24) + 1) == UNS and step(n_stop=65) == UNS
    assert step(batch=65536, stride=2) == BAD and step(ld=1 << 30, T=-1) == BAD and step(n_stop=65, tokens=None) == BAD      # a refusal comes first


def test_ngram_draft_statuses_without_device_work():
    lib = _lib.load()

    def draft(tokens=16, ld=20000, batch=3, total=32, nxt=48, T=9, min_n=1, max_n=4, out=64, root=80, cand=96, match=112, seq=128, rtl=144,
              ws=160, ws_bytes=36):
        return lib.mm_ngram_draft(tokens, ld, batch, total, nxt, T, min_n, max_n, out, root, cand, match, seq, rtl, ws, ws_bytes, None)

    assert draft(batch=0) == OK
    assert draft(batch=0, tokens=None, total=None, nxt=None, out=None, root=None, cand=None, match=None, seq=None, rtl=None, ws=None, ws_bytes=0) == OK
    for name in ("tokens", "total", "nxt", "out", "root"):
        assert draft(**{name: None}) == BAD, name
    assert draft(batch=-1) == BAD and draft(ld=0) == BAD and draft(T=-1) == BAD and draft(batch=0, ld=0) == BAD
    assert draft(min_n=0) == BAD and draft(min_n=-1) == BAD and draft(min_n=5, max_n=4) == BAD and draft(max_n=0) == BAD
    assert draft(ws=None) == BAD and draft(ws_bytes=35) == BAD and draft(ws_bytes=0) == BAD      # three parts of three sequences: 36 bytes
    for name in ("tokens", "total", "nxt", "out", "root", "cand", "match", "seq", "rtl", "ws"):
        for off in (1, 2, 3):
            assert draft(**{name: 192 + off}) == BAD, name
    assert draft(batch=65536, ws_bytes=1 << 30) == UNS and draft(ld=(1 << 24) + 1, ws_bytes=1 << 30) == UNS and draft(max_n=17) == UNS
    assert draft(min_n=17, max_n=17) == UNS and draft(max_n=17, min_n=0) == BAD and draft(batch=65536, T=-1) == BAD
    assert draft(max_n=17, tokens=None) == BAD                                                # a refusal comes before a limit


def test_the_workspace_size():
    size = _lib.load().mm_ngram_draft_workspace_bytes
    for B, ld, parts in ((1, 1, 1), (7, 8192, 1), (1, 8193, 2), (65, 16403, 3), (65535, 1 << 24, 2048), (3, 131072, 16)):
        want = 4 * B * parts if parts > 1 else 0
        assert size(B, ld) == want == mixedgemm.ngram_draft_workspace_bytes(B, ld), (B, ld)
    assert size(0, 100) == 0 and size(-1, 100) == 0 and size(3, 0) == 0 and size(3, -1) == 0
    assert size(65536, 20000) == 0 and size(3, (1 << 24) + 1) == 0


def test_python_argument_errors():
    z = lambda *s: torch.zeros(s, dtype=torch.int32)
    with pytest.raises(TypeError):
        mixedgemm.ngram_draft(None, z(2), z(3), 4)
    with pytest.raises(TypeError):
        mixedgemm.ngram_draft(z(2, 8).long(), z(2), z(3), 4)
    with pytest.raises(RuntimeError, match="ld_tok"):
        mixedgemm.ngram_draft(z(16), z(2), z(3), 4)
    with pytest.raises(ValueError, match="min_n"):
        mixedgemm.ngram_draft(z(2, 8), z(2), z(3), 4, min_n=0)
    with pytest.raises(ValueError, match="max_n"):
        mixedgemm.ngram_draft(z(2, 8), z(2), z(3), 4, max_n=17)
    with pytest.raises(RuntimeError, match="next_indptr"):
        mixedgemm.ngram_draft(z(2, 8), z(2), z(2), 4)
    with pytest.raises(RuntimeError, match="draft_tok"):
        mixedgemm.ngram_draft(z(2, 8), z(2), z(3), 4, draft_tok=z(5))
    with pytest.raises(TypeError):
        mixedgemm.ngram_draft(z(2, 8), z(2), z(3), 4, 1)                                     # min_n is keyword-only
    ok = (z(2, 8), z(2), z(2), z(2, 66), z(4), z(3), z(2), z(2))
    mixedgemm.token_step(*ok)
    for at, bad, err in ((1, z(3), RuntimeError), (2, z(2).long(), TypeError), (3, z(2, 65), RuntimeError), (4, z(2, 2), RuntimeError),
                         (5, z(2), RuntimeError), (6, z(1), RuntimeError), (7, None, TypeError)):
        args = list(ok)
        args[at] = bad
        with pytest.raises(err):
            mixedgemm.token_step(*args)
    with pytest.raises(RuntimeError, match="stop_tok"):
        mixedgemm.token_step(*ok, stop_tok=z(2, 65))
    with pytest.raises(RuntimeError, match="stop_tok"):
        mixedgemm.token_step(*ok, stop_tok=z(2))
    with pytest.raises(RuntimeError, match="emitted"):
        mixedgemm.token_step(*ok, emitted=z(3))


# ---- the CPU path against the oracle -----------------------------------------------------------------------------------------------------
def random_history_case(rng, B, ld):
    """a seeded small-alphabet state: histories over 3 tokens (a padding id among them), lengths from 0 to past the buffer"""
    tokens = [[rng.choice((0, 1, -1)) for _ in range(ld)] for _ in range(B)]
    total = [rng.choice((0, 1, 2, ld - 1, ld, ld + 3, -2)) if rng.random() < 0.3 else rng.randrange(ld + 1) for _ in range(B)]
    counts = [rng.choice((0, 1, 2, 5, 64, 65)) if rng.random() < 0.4 else rng.randrange(1, 9) for _ in range(B)]
    indptr = [0]
    for n in counts:
        indptr.append(indptr[-1] + n)
    return tokens, total, indptr


@pytest.mark.parametrize("seed", range(4))
def test_ngram_draft_on_cpu_tensors_equals_the_oracle(seed):
    rng = random.Random(seed)
    for case in range(60):
        B, ld = rng.randrange(1, 6), rng.choice((1, 2, 7, 40, 90))
        tokens, total, indptr = random_history_case(rng, B, ld)
        T = indptr[-1] if rng.random() < 0.8 else max(0, indptr[-1] - 3)             # a next_indptr that runs past num_tokens is clamped
        min_n = rng.randrange(1, 5)
        max_n = rng.randrange(min_n, 17)
        want_tokens = [row[:] for row in tokens]
        want = to.ngram_draft(want_tokens, total, indptr, T, min_n, max_n)
        t = i32(tokens)
        outs = {k: torch.full((T if k not in ("root_tok", "match_len") else B,), -7, dtype=torch.int32) for k in want}
        got = mixedgemm.ngram_draft(t, i32(total), i32(indptr), T, min_n=min_n, max_n=max_n, **outs)
        assert t.tolist() == want_tokens, (seed, case)
        for k, v in want.items():
            assert getattr(got, k) is outs[k] and outs[k].tolist() == [-7 if x is None else x for x in v], (seed, case, k)
    fresh = mixedgemm.ngram_draft(i32([[4, 5, 4, 0, 0, 0]]), i32([3]), i32([0, 3]), 3)
    assert fresh.draft_tok.tolist() == [4, 5, 4] and fresh.cand_tok.tolist() == [5, 4, -1] and fresh.match_len.tolist() == [1]
    assert fresh.root_tok.tolist() == [4] and fresh.row_seq.tolist() == [0, 0, 0] and fresh.row_total_len.tolist() == [3, 4, 5]


def random_step_case(rng, B, ld):
    tokens = [[rng.randrange(-1, 4) for _ in range(ld)] for _ in range(B)]
    total = [rng.choice((-1, 0, ld, ld + 2)) if rng.random() < 0.15 else rng.randrange(ld + 1) for _ in range(B)]
    finished = [rng.choice((0, 0, 0, 1, 2)) for _ in range(B)]
    counts = [rng.choice((0, 65, 70)) if rng.random() < 0.15 else rng.randrange(1, 9) for _ in range(B)]
    qo = [0]
    for n in counts:
        qo.append(qo[-1] + n)
    T = qo[-1]
    target = [rng.randrange(0, 4) for _ in range(T)]
    result = []
    for n in counts:
        k = rng.randrange(0, min(n, 64) + 1) if rng.random() < 0.9 else rng.choice((-1, n + 1, 70))
        path = sorted(rng.sample(range(n), k)) if 0 <= k <= min(n, 64) else [0] * min(max(k, 0), 64)
        if path and rng.random() < 0.05:
            path[-1] = n                                                              # a row verify_greedy does not write
        result.append([k, rng.randrange(4)] + path + [-1] * (64 - len(path)))
    root = [rng.choice((-1, 0, 2)) for _ in range(B)]
    most = [rng.choice((0, ld, ld + 5, -3)) if rng.random() < 0.2 else rng.randrange(ld + 1) for _ in range(B)]
    n_stop = rng.randrange(0, 4)
    stop = [[rng.randrange(-1, 4) for _ in range(n_stop)] for _ in range(B)] if n_stop else None
    return tokens, total, finished, result, target, qo, root, most, stop


@pytest.mark.parametrize("seed", range(4))
def test_token_step_on_cpu_tensors_equals_the_oracle(seed):
    rng = random.Random(100 + seed)
    for case in range(80):
        B, ld = rng.randrange(1, 6), rng.choice((1, 3, 12, 30))
        tokens, total, finished, result, target, qo, root, most, stop = random_step_case(rng, B, ld)
        kv = rng.choice((None, 0, 0, 7))
        w_tokens, w_total, w_fin = [r[:] for r in tokens], total[:], finished[:]
        want = to.token_step(w_tokens, w_total, w_fin, result, target, qo, root, most, stop, kv_status=kv or 0)
        t, tl, fin, em = i32(tokens), i32(total), i32(finished), torch.full((B,), -7, dtype=torch.int32)
        got = mixedgemm.token_step(t, tl, fin, i32(result), i32(target), i32(qo), i32(root), i32(most),
                                   stop_tok=None if stop is None else i32(stop), kv_state=None if kv is None else i32([kv, 0, 0, 0]), emitted=em)
        assert got is em and em.tolist() == ([-7] * B if want is None else want), (seed, case)
        assert (t.tolist(), tl.tolist(), fin.tolist()) == (w_tokens, w_total, w_fin), (seed, case)


# ---- the loop on CPU tensors ---------------------------------------------------------------------------------------------------------------
def loop_state(variant, device="cpu"):
    prompts, max_total, stops = to.loop_requests(variant)
    tokens = torch.full((len(prompts), to.LOOP_LD), -1, dtype=torch.int32)
    for b, p in enumerate(prompts):
        tokens[b, :len(p)] = i32(p)
    return (tokens.to(device), i32([len(p) for p in prompts]).to(device), torch.zeros(len(prompts), dtype=torch.int32, device=device),
            i32(max_total).to(device), i32(stops).to(device))


def check_loop(variant, tokens, total_len, finished, emitted, steps=to.LOOP_STEPS, accepted=True):
    """the speculative-decoding invariant: the committed tokens are the plain rollout's, whatever was drafted"""
    prompts = to.loop_requests(variant)[0]
    total, fin, rows = total_len.tolist(), finished.tolist(), tokens.tolist()
    for b, (h, end) in enumerate(to.loop_expected(variant)):
        assert rows[b][:total[b]] == h[:total[b]], f"sequence {b}"
        assert total[b] == len(prompts[b]) + sum(e[b] for e in emitted), f"sequence {b}: emitted"
        if fin[b]:
            assert (total[b], fin[b]) == (len(h), end), f"sequence {b} finished"
        else:
            assert total[b] < len(h) and total[b] >= min(len(h), len(prompts[b]) + steps), f"sequence {b}: a running sequence commits a token a step"
    if accepted:
        assert max(sum(e[b] for e in emitted) for b in range(len(prompts))) > steps, "no draft was ever accepted"
    return total, fin


def test_the_loop_on_cpu_tensors_is_the_plain_rollout():
    f = i32(to.model_table())
    indptr = [0]
    for n in to.LOOP_NODES:
        indptr.append(indptr[-1] + n)
    T, qo = indptr[-1], i32(indptr)
    seen = []
    for variant in (0, 1):
        tokens, total_len, finished, max_total, stops = loop_state(variant)
        emitted = []
        for _ in range(to.LOOP_STEPS):
            d = mixedgemm.ngram_draft(tokens, total_len, qo, T, min_n=1, max_n=4)
            target = f[d.draft_tok.long()]
            result = i32(to.chain_verify(target.tolist(), d.draft_tok.tolist(), d.root_tok.tolist(), indptr))
            emitted.append(mixedgemm.token_step(tokens, total_len, finished, result, target, qo, d.root_tok, max_total, stop_tok=stops).tolist())
        seen.append(check_loop(variant, tokens, total_len, finished, emitted))
    assert {1, 2} <= set(seen[0][1]) and 0 in seen[0][1], f"precondition: a stop, a limit and a running sequence: {seen[0]}"
