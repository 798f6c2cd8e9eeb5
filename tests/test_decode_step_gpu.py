"""GPU tests of the one-launch decode step (mixedgemm.rope_append_decode, PagedKVCache.decode_step; include/micromix_decode_step.h):
equality with rope_kv_append -> paged_decode on a poisoned twin cache, fp64, a page outside the cache, a replayed hipGraph."""
import numpy as np
import pytest
import torch

from micromix_amd import mixedgemm
from micromix_amd.kvcache import PagedKVCache
import kv_exact_cases as kc
import kv_fp8_oracle as fo
import kv_oracle as ko
import rope_oracle as ro
import test_kvcache_gpu as t_dec

pytestmark = pytest.mark.gpu

L, LAYER = 2, 1
KINDS = ["int4", "fp8_e4m3", "bf16"]
# the new token: absent, alone, on both sides of a 32-token tile, a 128-token round of the waves and a 256-token chunk, past the bound
LENS = [0, 1, 32, 33, 128, 129, 256, 257, 1024, 1100]


def i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def raw(t):
    return t.view(torch.int16) if t.element_size() == 2 else t


def poisoned_cache(kind, max_pages, Hkv, P, dev):
    if kind == "bf16":
        return torch.full((max_pages, L, 2, Hkv, P, 128), float("nan"), dtype=torch.bfloat16, device=dev), None
    data = torch.full((max_pages, L, 2, Hkv, P, 64 if kind == "int4" else 128), 0xFF, dtype=torch.uint8, device=dev)
    return data, torch.full((max_pages, L, 2, Hkv, P, 2), float("nan"), dtype=torch.float16, device=dev)


def step_inputs(lens, Hq, Hkv, dev, seed, q_scale=1.0, k_is_q=False):
    """q, k, v as views of one packed projection, cos / sin of each sequence's last position"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    B, g_heads = len(lens), Hq // Hkv
    packed = torch.randn((B, (Hq + 2 * Hkv) * 128), generator=g).to(torch.bfloat16)
    packed[:, : Hq * 128] *= q_scale
    if k_is_q:                                            # rope(k) = rope(q) of the group's first head: the new token takes the weight
        packed[:, Hq * 128: (Hq + Hkv) * 128] = packed[:, : Hq * 128].view(B, Hkv, g_heads, 128)[:, :, 0].reshape(B, Hkv * 128)
    packed = packed.to(dev)
    cos, sin = (torch.from_numpy(t.view(np.int16).copy()).view(torch.bfloat16).to(dev) for t in ro.llama3_tables([max(n - 1, 0) for n in lens]))
    return packed[:, : Hq * 128], packed[:, Hq * 128: (Hq + Hkv) * 128], packed[:, (Hq + Hkv) * 128:], cos, sin


def filled_twins(kind, lens, Hkv, P, dev, seed, bad_seq=None):
    """two poisoned caches holding the same len - 1 earlier tokens, and the step's page table; bad_seq: its last page entry is max_pages"""
    indptr, indices, last, max_pages = kc.page_table(lens, P, seed)
    prior = [max(n - 1, 0) for n in lens]
    prior_idx = np.concatenate([indices[indptr[b]: indptr[b] + -(-n // P)] for b, n in enumerate(prior)] + [np.zeros(0, np.int32)])
    prior_tbl = [i32(a, dev) for a in (kc.indptr_of([-(-n // P) for n in prior]), prior_idx, [n - (-(-n // P) - 1) * P if n else 0 for n in prior])]
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    k, v = (torch.randn((sum(prior), Hkv, 128), generator=g).to(torch.bfloat16).to(dev) for _ in range(2))
    caches = []
    for _ in range(2):
        data, param = poisoned_cache(kind, max_pages, Hkv, P, dev)
        mixedgemm.kv_append(data, param, *prior_tbl, k, v, i32(kc.indptr_of(prior), dev), LAYER)
        caches.append((data, param))
    if bad_seq is not None:
        indices = indices.copy()
        indices[indptr[bad_seq + 1] - 1] = max_pages
    return caches, (indptr, indices, last)


def run_both(kind, Hq, Hkv, P, lens, bounds, dev, seed, bad_seq=None):
    """the chain on one twin, the fused call on the other, once per bound (the step is idempotent); the chain's cache before and after"""
    (chain, fused), tbl_h = filled_twins(kind, lens, Hkv, P, dev, seed, bad_seq)
    tbl = [i32(a, dev) for a in tbl_h]
    q, k, v, cos, sin = step_inputs(lens, Hq, Hkv, dev, seed + 2)
    before = chain[0].clone()
    for bound in bounds:
        q_rot = mixedgemm.rope_kv_append(*chain, *tbl, q, k, v, cos, sin, i32(np.arange(len(lens) + 1), dev), LAYER)
        want = mixedgemm.paged_decode(q_rot, *chain, *tbl, LAYER, bound)
        q_out = torch.zeros_like(q_rot)
        got = mixedgemm.rope_append_decode(*fused, *tbl, q, k, v, cos, sin, LAYER, bound, q_out=q_out)
        assert torch.equal(raw(fused[0]), raw(chain[0])), f"bound {bound}: cache bytes differ"
        assert kind == "bf16" or torch.equal(raw(fused[1]), raw(chain[1])), f"bound {bound}: cache parameters differ"
        assert torch.equal(raw(q_out), raw(q_rot)), f"bound {bound}: rotated q differs"
        assert torch.isfinite(want.float()).all(), "the chain itself read poison"
        bad = (raw(got) != raw(want)).any(-1).nonzero().tolist()
        assert not bad, f"bound {bound}: o differs from the chain's in (sequence, head) {bad[:8]}"
    return before, chain[0]


@pytest.mark.parametrize("P", [1, 16, 24])
@pytest.mark.parametrize("Hq,Hkv", [(32, 8), (4, 4), (16, 1)])
@pytest.mark.parametrize("kind", KINDS)
def test_equals_the_chain(dev, kind, Hq, Hkv, P):
    """max_seq_len 1024: four chunks and the merge launch; 200: one chunk, no workspace"""
    assert mixedgemm.rope_append_decode_workspace_bytes(len(LENS), Hq, Hkv, 1024) == len(LENS) * Hq * 4 * 130 * 4
    assert mixedgemm.rope_append_decode_workspace_bytes(len(LENS), Hq, Hkv, 200) == 0
    before, after = run_both(kind, Hq, Hkv, P, LENS, (1024, 200), dev, 7 * P + Hq)
    assert (raw(before) != raw(after)).any(-1).sum() == 2 * Hkv * (len(LENS) - 1), "one K and one V row per kv head of every live sequence"


@pytest.mark.parametrize("kind", KINDS)
def test_against_fp64(dev, kind):
    """q of scale 2 and the new token's k along q: a step that skipped the new row, or attended a stale one, is far outside the bound"""
    Hq, Hkv, P, lens = 8, 2, 16, [1, 33, 257, 700]
    (_, cache), tbl_h = filled_twins(kind, lens, Hkv, P, dev, 50)
    q, k, v, cos, sin = step_inputs(lens, Hq, Hkv, dev, 51, q_scale=2.0, k_is_q=True)
    q_out = torch.zeros((len(lens), Hq, 128), dtype=torch.bfloat16, device=dev)
    o = mixedgemm.rope_append_decode(*cache, *(i32(a, dev) for a in tbl_h), q, k, v, cos, sin, LAYER, max(lens), q_out=q_out)
    torch.cuda.synchronize()
    data, param = cache[0].cpu(), None if kind == "bf16" else cache[1].cpu().numpy()
    if kind == "fp8_e4m3":
        data, param = fo.dequantize(data.numpy(), param), None
    else:
        data = data.view(torch.int16).numpy().view(np.uint16) if kind == "bf16" else data.numpy()
    want = ko.attention(raw(q_out).cpu().numpy().view(np.uint16), data, param, *tbl_h, LAYER)
    vmax = max(float(np.abs(ko.dequantized(data, param, *tbl_h, LAYER, b)[1]).max()) for b in range(len(lens)))
    t_dec.check_attention(o, want, vmax)


@pytest.mark.parametrize("kind", KINDS)
def test_page_outside_the_cache_is_neither_written_nor_attended(dev, kind):
    lens = [40, 49, 17]                                   # sequence 1: the new token alone on its last page, whose entry is max_pages
    before, after = run_both(kind, 8, 2, 16, lens, (64,), dev, 60, bad_seq=1)
    assert (raw(before) != raw(after)).any(-1).sum() == 2 * 2 * (len(lens) - 1), "the guarded sequence's rows must not be written"


def test_graph_replays_equal_the_eager_chain(dev):
    """two chunks (B * Hkv = 6, bound 512), so the captured step is the walk and the merge; a page is crossed on the way"""
    B, Hq, Hkv, P, bound = 3, 8, 2, 16, 512
    fused, chain = (PagedKVCache(L, Hkv, P, 24, B, kind="int4", device=dev, max_seq_len=bound) for _ in range(2))
    g = torch.Generator(device="cpu").manual_seed(70)
    first = [70, 5, 46]
    k0, v0 = (torch.randn((sum(first), Hkv, 128), generator=g).to(torch.bfloat16).to(dev) for _ in range(2))
    for c in (fused, chain):
        c.extend(first)
        c.append(LAYER, k0, v0)
        c.extend(1)
    q, k, v, cos, sin = step_inputs([n + 1 for n in first], Hq, Hkv, dev, 71)      # the buffers the graph reads, rewritten in place
    run = lambda: fused.decode_step(LAYER, q, k, v, cos, sin, max_seq_len=bound)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for step in range(4):
        if step:
            fused.extend(1)
            chain.extend(1)
        for dst, src in zip((q, k, v, cos, sin), step_inputs(fused.seq_lens, Hq, Hkv, dev, 72 + step)):
            dst.copy_(src)
        graph.replay()
        want = chain.attend(LAYER, chain.append_rope(LAYER, q, k, v, cos, sin), max_seq_len=bound)
        assert torch.equal(raw(out), raw(want)), f"replay {step}: o differs from the eager chain's"
        assert torch.equal(fused.kv_data, chain.kv_data) and torch.equal(raw(fused.kv_param), raw(chain.kv_param)), f"replay {step}: cache differs"
