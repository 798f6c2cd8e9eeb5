"""GPU tests of QK-norm in the three RoPE kernels (include/micromix_qknorm.h; qk_norm= of mixedgemm.rope_kv_append,
rope_kv_append_dense, rope_qk, rope_append_decode and PagedKVCache) against tests/qknorm_oracle.py.  Every comparison is bit equality.
The reference of a normed call: its rotated q is rope_oracle.rope of the oracle's normed q, on the CPU; its cache is what the plain
mixedgemm.kv_append -- pinned to the CPU cache oracles by its own tests, for all three kinds -- writes for rope(normed k) and v."""
import numpy as np
import pytest
import torch

from micromix_amd import mixedgemm
from micromix_amd.kvcache import PagedKVCache
import qknorm_oracle as qo
import rope_oracle as ro
import test_decode_step_gpu as t_step
from test_rope_append_gpu import bits, dev_i32, from_bits

pytestmark = pytest.mark.gpu
KINDS, LAYER = t_step.KINDS, t_step.LAYER
GAUSS = qo.gaussian_case()         # computed once, with its normed and rotated reference: the input that tells the tree from other orders
GAUSS_TABLES = ro.llama3_tables(np.arange(1024) * 61 % 4099)
GAUSS_WANT = tuple(ro.rope(qo.qknorm(x, w, GAUSS[5]), *GAUSS_TABLES) for x, w in ((GAUSS[0], GAUSS[3]), (GAUSS[1], GAUSS[4])))


def small_case(T, Hq, Hkv, seed, dev):
    """q, k, v as views of one packed projection, tables, weights; the normed and rotated q and k by the oracle"""
    rng = np.random.default_rng(seed)
    packed = from_bits(ro.f32_to_bf16(rng.standard_normal((T, (Hq + 2 * Hkv) * 128)).astype(np.float32) * np.float32(2.0)), dev)
    q, k, v = packed[:, : Hq * 128], packed[:, Hq * 128: (Hq + Hkv) * 128], packed[:, (Hq + Hkv) * 128:]
    tables = ro.llama3_tables(rng.integers(0, 131072, T))
    qw, kw = (ro.f32_to_bf16(1.0 + 0.25 * rng.standard_normal(128).astype(np.float32)) for _ in range(2))
    want = tuple(ro.rope(qo.qknorm(bits(x).reshape(T, -1, 128), w, 1e-5), *tables) for x, w in ((q, qw), (k, kw)))
    return (q, k, v), tuple(from_bits(t, dev) for t in tables), (from_bits(qw, dev), from_bits(kw, dev), 1e-5), want


def table(lens, P, dev, seed=0, bad_seq=None):
    """kv_exact_cases' shuffled page table for these lengths; bad_seq: its last page entry is -1 (no valid slot)"""
    indptr, indices, last, max_pages = t_step.kc.page_table(lens, P, seed)
    if bad_seq is not None:
        indices = indices.copy()
        indices[indptr[bad_seq + 1] - 1] = -1
    return [dev_i32(a, dev) for a in (indptr, indices, last)], max_pages


def same(a, b, kind, what):
    assert torch.equal(t_step.raw(a[0]), t_step.raw(b[0])), f"{what}: cache bytes differ"
    assert kind == "bf16" or torch.equal(t_step.raw(a[1]), t_step.raw(b[1])), f"{what}: cache parameters differ"


@pytest.mark.parametrize("g", [1, 4, 7])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_rope_kv_append(dev, kind, T, g):
    """P = 4: sequence 0 appends at positions 3.. and with T = 3 crosses a page; there the token of sequence 1 has no valid slot"""
    Hkv, P, new = 2, 4, [T - T // 2, T // 2]
    lens = [3 + new[0], 1 + new[1]]
    (q, k, v), (cos, sin), norm, (want_q, want_k) = small_case(T, g * Hkv, Hkv, 10 * T + g, dev)
    tbl, max_pages = table(lens, P, dev, bad_seq=1 if new[1] else None)
    app = dev_i32(np.array([0, new[0], T]), dev)
    got, want = (t_step.poisoned_cache(kind, max_pages, Hkv, P, dev) for _ in range(2))
    q_rot = mixedgemm.rope_kv_append(*got, *tbl, q, k, v, cos, sin, app, LAYER, qk_norm=norm)
    mixedgemm.kv_append(*want, *tbl, from_bits(want_k, dev), v.reshape(T, Hkv, 128).contiguous(), app, LAYER)
    assert np.array_equal(bits(q_rot), want_q), "q differs from the oracle"
    same(got, want, kind, "rope_kv_append(qk_norm=)")


@pytest.mark.parametrize("Hq,Hkv", [(4, 2), (8, 1), (64, 2)])
@pytest.mark.parametrize("T", [1, 7, 8, 9, 17])
def test_dense_and_rope_qk(dev, T, Hq, Hkv):
    """with a cache of each kind (k_out, v_out as the wrapper passes them) and without one (rope_qk: v_out NULL)"""
    (q, k, v), (cos, sin), norm, (want_q, want_k) = small_case(T, Hq, Hkv, 100 * T + Hq, dev)
    q_rot, k_rot = mixedgemm.rope_qk(q, k, cos, sin, qk_norm=norm)
    assert np.array_equal(bits(q_rot), want_q) and np.array_equal(bits(k_rot), want_k), "rope_qk differs from the oracle"
    tbl, max_pages = table([T], 4, dev)
    app = dev_i32(np.array([0, T]), dev)
    for kind in KINDS:
        got, want = (t_step.poisoned_cache(kind, max_pages, Hkv, 4, dev) for _ in range(2))
        q2, k_seen, v_seen = mixedgemm.rope_kv_append_dense(*got, *tbl, q, k, v, cos, sin, app, LAYER, qk_norm=norm)
        w_q, w_k, w_v = mixedgemm.rope_kv_append_dense(*want, *tbl, q, from_bits(want_k, dev), v, cos * 0 + 1, sin * 0, app, LAYER)
        assert np.array_equal(bits(q2), want_q), f"{kind}: q differs from the oracle"
        assert torch.equal(t_step.raw(k_seen), t_step.raw(w_k)) and torch.equal(t_step.raw(v_seen), t_step.raw(w_v)), f"{kind}: k_seen / v_seen"
        same(got, want, kind, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_the_kernels_realise_one_tree(dev, kind):
    """the large Gaussian input: all three kernels give the oracle's q and k, the first two byte for byte each other's cache"""
    q, k, v, qw, kw, eps = (from_bits(t, dev) if isinstance(t, np.ndarray) else t for t in GAUSS)
    cos, sin = (from_bits(t, dev) for t in GAUSS_TABLES)
    T, Hkv = q.size(0), k.size(1)
    tbl, max_pages = table([T], 16, dev)
    app = dev_i32(np.array([0, T]), dev)
    a, b, want = (t_step.poisoned_cache(kind, max_pages, Hkv, 16, dev) for _ in range(3))
    q_a = mixedgemm.rope_kv_append(*a, *tbl, q, k, v, cos, sin, app, LAYER, qk_norm=(qw, kw, eps))
    q_b = mixedgemm.rope_kv_append_dense(*b, *tbl, q, k, v, cos, sin, app, LAYER, qk_norm=(qw, kw, eps))[0]
    mixedgemm.kv_append(*want, *tbl, from_bits(GAUSS_WANT[1], dev), v, app, LAYER)
    assert np.array_equal(bits(q_a), GAUSS_WANT[0]) and np.array_equal(bits(q_b), GAUSS_WANT[0]), "q differs from the oracle's tree"
    same(a, want, kind, "rope_kv_append against the oracle's k")
    same(b, a, kind, "rope_kv_append_dense against rope_kv_append")
    tbl, max_pages = table([1] * T, 1, dev)                    # the decode step: the same tokens as T sequences of one token, g = 16
    c, want = (t_step.poisoned_cache(kind, max_pages, Hkv, 1, dev) for _ in range(2))
    q_c = torch.zeros_like(q)
    mixedgemm.rope_append_decode(*c, *tbl, q, k, v, cos, sin, LAYER, 1, q_out=q_c, qk_norm=(qw, kw, eps))
    mixedgemm.kv_append(*want, *tbl, from_bits(GAUSS_WANT[1], dev), v, dev_i32(np.arange(T + 1), dev), LAYER)
    assert np.array_equal(bits(q_c), GAUSS_WANT[0]), "the decode step's q_out differs from the oracle's tree"
    same(c, want, kind, "the decode step's K rows against the oracle's k")


@pytest.mark.parametrize("g", [1, 4, 16])
@pytest.mark.parametrize("lens", [[5], [256, 257, 1100]], ids=["B1", "B3"])
@pytest.mark.parametrize("kind", KINDS)
def test_decode_step_equals_the_chain(dev, kind, lens, g):
    """bound 1024, which test_decode_step_gpu splits into chunks of 256: the new position in the first chunk (5), at a chunk's last
    and first place (256, 257), in the last chunk past the bound (1100)"""
    Hkv, P = 2, 16
    (chain, fused), tbl_h = t_step.filled_twins(kind, lens, Hkv, P, dev, 30 + g)
    tbl = [dev_i32(a, dev) for a in tbl_h]
    (q, k, v), (cos, sin), norm, (want_q, _) = small_case(len(lens), g * Hkv, Hkv, 40 + g, dev)
    q_rot = mixedgemm.rope_kv_append(*chain, *tbl, q, k, v, cos, sin, dev_i32(np.arange(len(lens) + 1), dev), LAYER, qk_norm=norm)
    want = mixedgemm.paged_decode(q_rot, *chain, *tbl, LAYER, 1024)
    q_out = torch.zeros_like(q_rot)
    got = mixedgemm.rope_append_decode(*fused, *tbl, q, k, v, cos, sin, LAYER, 1024, q_out=q_out, qk_norm=norm)
    same(fused, chain, kind, "decode step")
    assert np.array_equal(bits(q_out), want_q) and torch.equal(t_step.raw(q_out), t_step.raw(q_rot)), "q_out"
    assert torch.isfinite(want.float()).all() and torch.equal(t_step.raw(got), t_step.raw(want)), "o differs from the chain's"


def test_graph_replay_after_weights_and_inputs_were_rewritten(dev):
    B, Hq, Hkv, bound = 3, 8, 2, 512
    fused, chain = (PagedKVCache(2, Hkv, 16, 24, B, kind="int4", device=dev, max_seq_len=bound) for _ in range(2))
    (q, k, v), (cos, sin), norm, _ = small_case(B, Hq, Hkv, 80, dev)
    for c in (fused, chain):
        c.extend([70, 5, 46])
        c.append(LAYER, *(torch.ones((121, Hkv, 128), dtype=torch.bfloat16, device=dev),) * 2)
        c.extend(1)
    run = lambda: fused.decode_step(LAYER, q, k, v, cos, sin, max_seq_len=bound, qk_norm=norm)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    (q2, k2, v2), (cos2, sin2), norm2, _ = small_case(B, Hq, Hkv, 81, dev)
    for dst, src in zip((q, k, v, cos, sin, norm[0], norm[1]), (q2, k2, v2, cos2, sin2, norm2[0], norm2[1])):
        dst.copy_(src)
    want = chain.attend(LAYER, chain.append_rope(LAYER, q2, k2, v2, cos2, sin2, qk_norm=norm2), max_seq_len=bound)
    for replay in range(2):                                   # the step is idempotent
        graph.replay()
        assert torch.equal(t_step.raw(out), t_step.raw(want)), f"replay {replay}: o differs from the eager chain's"
        same((fused.kv_data, fused.kv_param), (chain.kv_data, chain.kv_param), "int4", f"replay {replay}")


def test_qk_norm_none_gives_todays_bits(dev):
    """weight 1 with a row whose mean square is 1 would also pass through; None must not norm at all: against the un-normed oracle"""
    (q, k, v), (cos, sin), _, _ = small_case(3, 8, 2, 90, dev)
    want_q, want_k = (ro.rope(bits(x).reshape(3, -1, 128), bits(cos), bits(sin)) for x in (q, k))
    tbl, max_pages = table([1, 1, 1], 4, dev)
    caches = [t_step.poisoned_cache("bf16", max_pages, 2, 4, dev) for _ in range(4)]
    app = dev_i32(np.arange(4), dev)
    q_out = torch.zeros((3, 8, 128), dtype=torch.bfloat16, device=dev)
    mixedgemm.rope_append_decode(*caches[2], *tbl, q, k, v, cos, sin, LAYER, 4, q_out=q_out, qk_norm=None)
    for got in (mixedgemm.rope_kv_append(*caches[0], *tbl, q, k, v, cos, sin, app, LAYER, qk_norm=None),
                mixedgemm.rope_kv_append_dense(*caches[1], *tbl, q, k, v, cos, sin, app, LAYER, qk_norm=None)[0], q_out,
                mixedgemm.rope_qk(q, k, cos, sin, qk_norm=None)[0]):
        assert np.array_equal(bits(got), want_q)
    mixedgemm.kv_append(*caches[3], *tbl, from_bits(want_k, dev), v.reshape(3, 2, 128).contiguous(), app, LAYER)
    for c in caches[:3]:
        same(c, caches[3], "bf16", "qk_norm=None")
