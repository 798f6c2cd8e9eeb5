"""GPU tests of shared-prefix decode (mixedgemm.paged_decode_shared, PagedKVCache.attend(shared=True); include/micromix_hip.h,
mm_paged_decode_shared) against the fp64 oracle of tests/kv_oracle.py over the dequantized cache, within test_kvcache_gpu.py's own
check_attention budget: 2 bf16 ulps of the oracle value or 1e-3 max|V|.  The tables are built by hand (tests/kv_shared_oracle.py) so that
groups share real pages; every cache is NaN outside the rows its sequences hold.

Nothing here skips when the library lacks the entry point: without it every test fails."""
import functools

import numpy as np
import pytest
import torch

from micromix_amd import mixedgemm
from micromix_amd.kvcache import PagedKVCache
import kv_exact_cases as kc
import kv_shared_oracle as so
import test_kvcache_gpu as t_dec

pytestmark = pytest.mark.gpu

L, LAYER, HKV = 2, 1, 2
G_VALUES = (1, 3, 4, 8, 16)


def i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def to_dev(kind, data, param, dev):
    if kind == "bf16":
        return torch.from_numpy(data.view(np.int16)).to(dev).view(torch.bfloat16), None
    return torch.from_numpy(data).to(dev), torch.from_numpy(param).to(dev)


def bf(x, dev):
    return torch.from_numpy(kc.bf16_bits(x).view(np.int16)).to(dev).view(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def gaussian_case(kind, g, P, Hkv=HKV, groups=None, seed=None):
    """(layout, host image, q, fp64 reference, max|V|), computed once and shared by the tests that use the case; never modified"""
    seed = 1000 * g + 10 * P + len(kind) if seed is None else seed
    lay = so.layout(P, list(groups) if groups else so.random_groups(g, seed), seed)
    Kp, Vp = so.gaussian_rows(lay, Hkv, seed + 1)
    data, param = so.image(kind, lay, L, LAYER, Kp, Vp)
    q = kc.to_bf16(np.random.default_rng(seed + 2).standard_normal((lay["B"], g * Hkv, 128)).astype(np.float32) * 2.0)
    want = so.reference(kind, kc.bf16_bits(q), data, param, so.table(lay), LAYER)
    return lay, data, param, q, want, float(np.abs(Vp[lay["valid"]]).max())


def run(kind, lay, data, param, q, dev, max_shared=None, max_suffix=None, workspace=None):
    d, p = to_dev(kind, data, param, dev)
    o = mixedgemm.paged_decode_shared(bf(q, dev), d, p, *(i32(a, dev) for a in so.table(lay)), LAYER,
                                      *(i32(a, dev) for a in so.group_tables(lay)),
                                      lay["max_shared"] if max_shared is None else max_shared,
                                      lay["max_suffix"] if max_suffix is None else max_suffix, workspace=workspace)
    torch.cuda.synchronize()
    return o


# ---- 1. random caches against the oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 5, 16])
@pytest.mark.parametrize("g", G_VALUES)
@pytest.mark.parametrize("kind", so.KINDS)
def test_random_groups_against_fp64(dev, kind, g, P):
    lay, data, param, q, want, vmax = gaussian_case(kind, g, P)
    sizes = sorted({len(t) for _, t in lay["groups"]})
    assert sizes == sorted(set(so.group_sizes(g))) and any(s % P for s, _ in lay["groups"]) == (P > 1)
    assert 0 in lay["lens"] and not np.array_equal(lay["group_members"], np.arange(lay["B"]))
    assert any(t == 0 and s > 0 for s, tails in lay["groups"] for t in tails), "a member whose length is its shared count"
    o = run(kind, lay, data, param, q, dev)
    for b, n in enumerate(lay["lens"]):
        if n == 0:
            assert int(torch.count_nonzero(o[b].float())) == 0
    t_dec.check_attention(o, want, vmax)


# ---- 2. exact answers --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,shared", [(16, 33), (5, 33), (16, 32), (1, 31), (16, 128), (5, 129), (16, 1)])
@pytest.mark.parametrize("g", [1, 3, 4, 8])
@pytest.mark.parametrize("kind", so.KINDS)
def test_needle_names_its_token_across_the_seam(dev, kind, g, P, shared):
    """every query names the one token it must return (tests/kv_exact_cases.py's needle, to 2^-20): in one slab some members look for the
    first or the last shared token, others for the first or the last token of their own tail, and the heads of a member for different
    ones, so a wrong row-to-(member, head) mapping or an off-by-one at the seam returns another token outright"""
    per = 16 // g
    tails = [so.TAILS[(m + 1) % 4] for m in range(min(2 * per + 1, 9))]
    lay = so.layout(P, [(shared, tails), (0, [0]), (shared, [33])], seed=g + P)
    Kp, Vp = so.needle_rows(lay, HKV)
    q, expect, targets = so.needle_queries(lay, g, HKV, Vp)
    kinds = {("shared" if t < s else "tail") for b, s in enumerate(lay["shared_len"]) for t in targets[b] if t >= 0}
    assert kinds == {"shared", "tail"}
    assert all(len(set(targets[b])) > 1 for b in range(lay["B"]) if lay["lens"][b] > 1), "the heads of a member name different tokens"
    first_slab = lay["group_members"][:min(per, len(tails))]
    assert len({tuple(targets[b]) for b in first_slab}) >= min(3, len(first_slab)), "the members of a slab name different tokens"
    data, param = so.image(kind, lay, L, LAYER, Kp, Vp)
    o = run(kind, lay, data, param, q, dev).float().cpu().numpy().astype(np.float64)
    Hq = g * HKV
    label = lambda i: f"sequence {i // Hq} (shared {lay['shared_len'][i // Hq]}, length {lay['lens'][i // Hq]}) head {i % Hq} target {targets[i // Hq, i % Hq]}"
    msg = kc.describe_mismatch(o.reshape(-1, 128), expect.reshape(-1, 128), label, kc.EXACT_BOUND)
    assert msg is None, msg


# ---- 3. split paths ----------------------------------------------------------------------------------------------------------------------
SPLIT_GROUPS = ((300, (0, 1, 290, 33, 130)), (129, (130,)), (0, (0,)), (0, (259,)))


@pytest.mark.parametrize("bounds", [(1024, 1024), (512, 512), (256, 128)])
@pytest.mark.parametrize("kind", so.KINDS)
def test_split_prefix_and_split_tails(dev, kind, bounds):
    """one kv head: bounds of 1024 tokens cut both ranges into several chunks; bounds below the real counts (256 < 300 shared, 128 < 290
    of tail) leave the rest to the last chunk"""
    g = 4
    lay, data, param, q, want, vmax = gaussian_case(kind, g, 16, Hkv=1, groups=SPLIT_GROUPS, seed=77)
    ws = lambda a, b: mixedgemm.paged_decode_shared_workspace_bytes(lay["B"], g, 1, a, b)
    assert ws(128, 128) == lay["B"] * g * 2 * 130 * 4, "one chunk of each kind"
    assert ws(1024, 128) > ws(128, 128) and ws(128, 1024) > ws(128, 128) and ws(1024, 1024) > max(ws(1024, 128), ws(128, 1024))
    assert ws(*bounds) >= ws(128, 128)
    o = run(kind, lay, data, param, q, dev, *bounds)
    t_dec.check_attention(o, want, vmax)


# ---- 4. poison ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g,P", [(3, 5), (4, 16), (16, 1)])
@pytest.mark.parametrize("kind", so.KINDS)
def test_nan_workspace_and_nan_outside_the_sequences(dev, kind, g, P):
    """the workspace is NaN before the call, and so is every cache row no sequence holds (other pages, rows past the lengths, the
    other layer).  Finite outputs within budget: every partial the merge read was written by this call"""
    lay, data, param, q, want, vmax = gaussian_case(kind, g, P)
    assert not lay["valid"].all() and not lay["valid"][0].any()
    need = mixedgemm.paged_decode_shared_workspace_bytes(lay["B"], g * HKV, HKV, lay["max_shared"], lay["max_suffix"])
    ws = torch.full((need // 4 + 64,), float("nan"), dtype=torch.float32, device=dev)
    o = run(kind, lay, data, param, q, dev, workspace=ws)
    assert bool(torch.isfinite(o.float()).all())
    t_dec.check_attention(o, want, vmax)
    assert bool(torch.isnan(ws[need // 4:]).all()), "nothing written past the workspace's size"


# ---- 5. the cache class ------------------------------------------------------------------------------------------------------------------
def host_reference(kind, cache, q, layer):
    hd = cache.kv_data.cpu()
    hd = hd.view(torch.int16).numpy().view(np.uint16) if kind == "bf16" else hd.numpy()
    hp = cache.kv_param.cpu().numpy() if cache.kv_param is not None else None
    tbl = (cache.kv_indptr.cpu().numpy(), cache.kv_indices.cpu().numpy(), cache.last_page_len.cpu().numpy())
    return so.reference(kind, t_dec.bits(q), hd, hp, tbl, layer)


class Twins:
    """`a` attends both ways; `b` goes through the same fork / extend / truncate and never takes the new path"""

    def __init__(self, dev, kind, P, g, batch, seed):
        self.dev, self.kind, self.Hq, self.batch = dev, kind, g * HKV, batch
        self.a, self.b = (PagedKVCache(L, HKV, P, 96, batch, kind=kind, device=dev, max_seq_len=256) for _ in range(2))
        self.rng = np.random.default_rng(seed)

    def both(self, op, *args):
        for c in (self.a, self.b):
            getattr(c, op)(*args)
        if op == "extend":
            for layer in range(L):
                k, v = (t_dec.rand_bf16((self.a.num_new_tokens, HKV, 128), self.rng, self.dev, s) for s in (1.0, 0.5))
                self.a.append(layer, k, v)
                self.b.append(layer, k, v)
        self.check(f"{op}{args}")

    def check(self, what):
        q = t_dec.rand_bf16((self.batch, self.Hq, 128), self.rng, self.dev, 2.0)
        o = self.a.attend(LAYER, q, shared=True)
        plain, twin = self.a.attend(LAYER, q), self.b.attend(LAYER, q)
        torch.cuda.synchronize()
        assert torch.equal(plain.view(torch.int16), twin.view(torch.int16)), f"{what}: attend() differs from the cache that never shared"
        t_dec.check_attention(o, host_reference(self.kind, self.a, q, LAYER), 4.0)


@pytest.mark.parametrize("kind", so.KINDS)
def test_cache_class_script(dev, kind):
    t = Twins(dev, kind, 16, 4, 7, seed=len(kind))
    t.check("empty cache")
    t.both("extend", [37, 0, 0, 0, 0, 5, 0])
    for dst in (1, 2, 3, 4):
        t.both("fork", 0, dst)
    assert t.a.share_groups() == ([[0, 1, 2, 3, 4], [5], [6]], [37] * 5 + [0, 0])     # five members: a full slab and one more
    t.both("extend", 1)                                   # four copies; the shared count falls to 32
    assert t.a.share_groups()[1][:5] == [32] * 5 and t.a._max_suffix == 6
    t.both("extend", [3, 1, 0, 2, 40, 1, 0])
    t.both("truncate", 2, 20)
    assert t.a.share_groups()[1][:5] == [20] * 5
    t.both("fork", 5, 3)                                  # 3 leaves the big group for 5's
    assert t.a.share_groups()[0] == [[0, 1, 2, 4], [3, 5], [6]]
    t.both("reset", 0)                                    # the leader goes; 1 leads
    assert t.a.share_groups()[0] == [[0], [1, 2, 4], [3, 5], [6]]
    t.both("extend", [130, 1, 1, 0, 1, 1, 1])


# ---- 6. graph ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", so.KINDS)
def test_one_graph_while_the_groups_change(dev, kind):
    B, g = 5, 4
    Hq, bound = g * HKV, 256
    cache = PagedKVCache(L, HKV, 16, 128, B, kind=kind, device=dev, max_seq_len=bound)
    rng = np.random.default_rng(5)
    cache.extend([40, 0, 0, 5, 0])
    for layer in range(L):
        cache.append(layer, t_dec.rand_bf16((45, HKV, 128), rng, dev), t_dec.rand_bf16((45, HKV, 128), rng, dev, 0.5))
    sk, sv, sq = (t_dec.rand_bf16((B, h, 128), rng, dev) for h in (HKV, HKV, Hq))
    cache.extend(1)                                       # captured before anything is shared
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        cache.append(LAYER, sk, sv)
        cache.attend(LAYER, sq, max_seq_len=bound, shared=True, max_shared_len=bound)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cache.append(LAYER, sk, sv)
        out = cache.attend(LAYER, sq, max_seq_len=bound, shared=True, max_shared_len=bound)

    def replay(what, groups):
        assert cache.share_groups()[0] == groups, what
        for t in (sk, sv, sq):
            t.copy_(t_dec.rand_bf16(tuple(t.shape), rng, dev, 0.5 if t is sv else 1.0))
        graph.replay()
        torch.cuda.synchronize()
        t_dec.check_attention(out.clone(), host_reference(kind, cache, sq, LAYER), 4.0)

    replay("nothing shared", [[0], [1], [2], [3], [4]])
    cache.fork(0, 1)
    cache.fork(0, 2)
    cache.extend(1)                                       # a copying extend: 42 tokens, the shared count 32
    assert cache.share_groups()[1] == [32, 32, 32, 0, 0]
    replay("after a copying extend", [[0, 1, 2], [3], [4]])
    cache.fork(0, 4)                                      # forks that change the groups: 4 joins, and 2 keeps 20 tokens of 1
    cache.fork(1, 2, 20)
    cache.extend(1)
    assert cache.share_groups()[1] == [16, 16, 16, 0, 16]
    replay("after forks that change the groups", [[0, 1, 2, 4], [3]])
    cache.reset(0)                                        # the leader's reset dissolves its group into [1, 2, 4]
    cache.reset(3)
    cache.extend(1)
    replay("after resets", [[0], [1, 2, 4], [3]])


# ---- 7. wrapper errors -------------------------------------------------------------------------------------------------------------------
def test_wrapper_errors(dev):
    lay, data, param, q, want, vmax = gaussian_case("bf16", 4, 16)
    d, p = to_dev("bf16", data, param, dev)
    tbl = [i32(a, dev) for a in so.table(lay)]
    gi, gm, sl = (i32(a, dev) for a in so.group_tables(lay))
    qd = bf(q, dev)
    call = lambda *grp, **kw: mixedgemm.paged_decode_shared(kw.pop("q", qd), d, p, *tbl, LAYER, *grp, lay["max_shared"], lay["max_suffix"], **kw)
    with pytest.raises(TypeError, match="group_members"):
        call(gi, gm.long(), sl)
    with pytest.raises(TypeError, match="shared_len"):
        call(gi, gm, sl.float())
    with pytest.raises(RuntimeError, match="group_indptr"):
        call(gi[:-1], gm, sl)
    with pytest.raises(RuntimeError, match="group_members"):
        call(gi, gm.view(1, -1), sl)
    with pytest.raises(RuntimeError, match="shared_len"):
        call(gi, gm, torch.cat([sl, sl]))
    with pytest.raises(RuntimeError, match="group_indptr"):
        call(gi.cpu(), gm, sl)
    with pytest.raises(RuntimeError, match="workspace"):
        call(gi, gm, sl, workspace=torch.empty((64,), dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match="2\\^29"):
        mixedgemm.paged_decode_shared(qd, d, p, *tbl, LAYER, gi, gm, sl, -1, 0)
    q17 = torch.zeros((lay["B"], 17 * HKV, 128), dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError, match="unsupported configuration"):
        call(gi, gm, sl, q=q17)
    assert mixedgemm.paged_decode_shared_workspace_bytes(4, 17 * HKV, HKV, 100, 100) == 0
    out = torch.empty((lay["B"], 4 * HKV, 128), dtype=torch.bfloat16, device=dev)
    assert call(gi, gm, sl, out=out) is out
    torch.cuda.synchronize()
    t_dec.check_attention(out, want, vmax)
