"""GPU tests of the paged KV cache on pages that start past 2^31 and 2^32 bytes of the pool: one pool per kind (int4, fp8, bf16) whose
data tensor is just over 4 GiB (far_cases.POOLS), from torch.empty; only the pages a case names are ever written, and only by the
library.  Every page list mixes page 0, the first page wholly past 2^31 bytes, the first wholly past 2^32 bytes and the last page,
and page 1, which is where a 32-bit offset of the last page lands (tests/test_far_cpu.py).  The fp16 params of the int4 and fp8 pools
(0.25 and 0.125 GiB) cross no threshold; a pool whose params pass 2^31 bytes needs 32 GiB of data and is not built.

Each case has a twin: the same calls on a cache of nine pages that starts as a copy of the pool's named pages, with the page ids
remapped to 0 .. 8.  The far pages must equal the twin's byte for byte and every output the twin's bit for bit; the twin is held to
the oracles as the existing tests do (bytes exactly; attention within the bounds of tests/test_kvcache_gpu.py and
tests/test_kvprefill_gpu.py).

kv_append and rope_kv_append; paged_decode with the window off and on; paged_decode_shared; paged_prefill causal and tree-masked;
kv_copy_pages far -> near, near -> far and far -> far; kv_move_rows between far pages, with the neighbours of every far page compared."""
import numpy as np
import pytest
import torch

from micromix_amd import mixedgemm
import far_cases as fc
import kv_fp8_oracle as fo
import kv_oracle as ko
import kv_prefill_oracle as kpo
import rope_oracle as ro
import test_kvcache_gpu as t_dec
import test_kvprefill_gpu as t_pre

pytestmark = pytest.mark.gpu

HQ = 4
i32 = lambda a, dev: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def bf16(bits, dev):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)


def bits_of(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def raw(t):
    """a cache tensor's pages as host integers: uint16 for bf16 and fp16, uint8 otherwise"""
    return bits_of(t) if t.dtype in (torch.bfloat16, torch.float16) else t.detach().cpu().numpy()


class Case:
    """the pool of one kind, its twin, and the two sequences of every case: sequence 0 on pages [first past B32, 0, last, first past
    B31] with 57 tokens, sequence 1 sharing the first two of them and ending on page 1, 43 tokens"""

    def __init__(self, kind, dev):
        g = self.g = fc.POOLS[kind]
        self.kind, self.dev = kind, dev
        width, dtype = {"int4": (64, torch.uint8), "fp8": (128, torch.uint8), "bf16": (128, torch.bfloat16)}[kind]
        shape = (g.L, 2, g.Hkv, g.P)
        self.data = torch.empty((g.max_pages,) + shape + (width,), dtype=dtype, device=dev)
        self.param = None if kind == "bf16" else torch.empty((g.max_pages,) + shape + (2,), dtype=torch.float16, device=dev)
        assert self.data.numel() * self.data.element_size() == g.data_bytes() > fc.B32
        p0, p31, p32, last, p1 = g.pages()
        assert (p0, p1) == (0, 1) and g.far_pages() == [p0, p31, p32, last]
        self.named = g.pages() + g.spare_pages()                                  # twin page i holds pool page named[i]
        assert len(set(self.named)) == len(self.named) == 8 and max(self.named) < g.max_pages
        self.near = {p: i for i, p in enumerate(self.named)}
        sel = torch.tensor(self.named, device=dev)
        self.twin_data = torch.cat([self.data[sel], torch.zeros_like(self.data[:1])])
        self.twin_param = None if self.param is None else torch.cat([self.param[sel], torch.zeros_like(self.param[:1])])
        self.seq_pages = [[p32, p0, last, p31], [p32, p0, p1]]
        self.lens = [57, 43]
        self.shared = 32
        self.new = [7, 11]                                                        # the tokens of the second append and of the prefill

    def tables(self, seqs=(0, 1), lens=None, near=False):
        """(kv_indptr, kv_indices, last_page_len) on the host for the named sequences at the given lengths"""
        lens = [self.lens[s] for s in seqs] if lens is None else lens
        P = self.g.P
        pages = [self.seq_pages[s][: -(-n // P)] for s, n in zip(seqs, lens)]
        idx = [self.near[p] if near else p for pl in pages for p in pl]
        assert all(0 <= p < self.g.max_pages for pl in pages for p in pl)
        return (np.concatenate([[0], np.cumsum([len(p) for p in pages])]).astype(np.int32), np.array(idx, dtype=np.int32),
                np.array([n - (len(p) - 1) * P for n, p in zip(lens, pages)], dtype=np.int32))

    def both(self, seqs=(0, 1), lens=None):
        """[(data, param, device page table)] of the pool and of the twin"""
        return [(d, p, [i32(a, self.dev) for a in self.tables(seqs, lens, near)])
                for d, p, near in ((self.data, self.param, False), (self.twin_data, self.twin_param, True))]

    def host_twin(self):
        return raw(self.twin_data).copy(), None if self.twin_param is None else self.twin_param.cpu().numpy().copy()

    def oracle_append(self):
        return fo.append if self.kind == "fp8" else ko.append

    def assert_far_equals_twin(self, what):
        sel = torch.tensor(self.named, device=self.dev)
        n = len(self.named)
        for name, far, twin in (("data", self.data, self.twin_data), ("param", self.param, self.twin_param)):
            if far is not None:
                a, b = raw(far[sel]), raw(twin[:n])
                bad = (a != b).reshape(n, -1).any(axis=1)
                assert not bad.any(), f"{what}: {name} of pool pages {[self.named[i] for i in np.flatnonzero(bad)]} differ from the twin's"

    def assert_twin_is(self, want_d, want_p, what):
        assert np.array_equal(raw(self.twin_data), want_d), f"{what}: the twin's data differ from the oracle's"
        assert want_p is None or np.array_equal(raw(self.twin_param), want_p.view(np.uint16)), f"{what}: the twin's params differ from the oracle's"

    def dequantized_twin(self):
        """(kv_data, kv_param) of the twin as tests/kv_oracle.py's attention takes them, zero outside the sequences' tokens (the pool
        came from torch.empty); an fp8 cache as the bf16 bits it decodes to"""
        hd, hp = self.host_twin()
        cd, cp = np.zeros_like(hd), None if hp is None else np.zeros_like(hp)
        for pages, n in zip(self.seq_pages, self.lens):
            for i, page in enumerate(pages):
                m = min(self.g.P, n - i * self.g.P)
                cd[self.near[page], :, :, :, :m] = hd[self.near[page], :, :, :, :m]
                if hp is not None:
                    cp[self.near[page], :, :, :, :m] = hp[self.near[page], :, :, :, :m]
        return (fo.dequantize(cd, cp), None) if self.kind == "fp8" else (cd, cp)

    def v_max(self, hd, hp, layer):
        tbl = self.tables(near=True)
        return max(float(np.abs(ko.dequantized(hd, hp, *tbl, layer, b)[1]).max()) for b in range(2))


@pytest.fixture(scope="module", params=["int4", "fp8", "bf16"])
def case(request, dev):
    """one pool at a time, filled by kv_append in two steps (sequence 0's first 50 tokens, then 7 and 11 new ones), both layers"""
    need, free = fc.POOLS[request.param].need_bytes(), torch.cuda.mem_get_info(dev)[0]
    if free < need:
        pytest.skip(f"the far {request.param} pool needs {need / fc.GIB:.1f} GiB of device memory (tests/far_cases.py), "
                    f"{free / fc.GIB:.1f} GiB are free")
    box = [Case(request.param, dev)]
    yield box[0]
    box[0].__dict__.clear()
    box.clear()
    torch.cuda.empty_cache()


def rows(rng, n, heads, scale):
    return fc.bf16_bits(rng.standard_normal((n, heads, 128)) * scale)


def append_steps(c):
    """[(sequences, lengths after the step, tokens appended per sequence)]"""
    return [((0,), [c.lens[0] - c.new[0]], [c.lens[0] - c.new[0]]), ((0, 1), c.lens, c.new)]


def fill(c, rope):
    """append every token of both sequences to both layers of the pool and of the twin; the oracle applied to the twin's first state"""
    rng = np.random.default_rng(len(c.kind) + rope)
    want_d, want_p = c.host_twin()
    for layer in range(c.g.L):
        for seqs, lens, new in append_steps(c):
            T = sum(new)
            kb, vb, qb = rows(rng, T, c.g.Hkv, 2.0), rows(rng, T, c.g.Hkv, 0.5), rows(rng, T, HQ, 1.0)
            app = np.concatenate([[0], np.cumsum(new)]).astype(np.int32)
            first = [n - m for n, m in zip(lens, new)]
            cos, sin = ro.llama3_tables(np.concatenate([np.arange(a, n) for a, n in zip(first, lens)]))
            q_rot = []
            for data, param, tbl in c.both(seqs, lens):
                if rope:
                    q_rot.append(mixedgemm.rope_kv_append(data, param, *tbl, bf16(qb, c.dev), bf16(kb, c.dev), bf16(vb, c.dev), bf16(cos, c.dev),
                                                          bf16(sin, c.dev), i32(app, c.dev), layer))
                else:
                    mixedgemm.kv_append(data, param, *tbl, bf16(kb, c.dev), bf16(vb, c.dev), i32(app, c.dev), layer)
            if rope:
                assert torch.equal(q_rot[0].view(torch.int16), q_rot[1].view(torch.int16))
                assert np.array_equal(bits_of(q_rot[0]), ro.rope(qb, cos, sin)), "the rotated q"
                kb = ro.rope(kb, cos, sin)
            c.oracle_append()(want_d, want_p, *c.tables(seqs, lens, near=True), kb, vb, app, layer)
    torch.cuda.synchronize()
    what = "rope_kv_append" if rope else "kv_append"
    c.assert_far_equals_twin(what)
    c.assert_twin_is(want_d, want_p, what)
    c.filled = True


def filled(c):
    if not getattr(c, "filled", False):
        fill(c, rope=False)
    return c


def test_kv_append(case):
    fill(case, rope=False)


def test_rope_kv_append(case):
    fill(case, rope=True)


def same(outs, what):
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), f"{what}: the far pool's output differs from the twin's"


@pytest.mark.parametrize("window", [None, 24])
def test_paged_decode(case, window):
    c = filled(case)
    qb = rows(np.random.default_rng(3), 2, HQ, 2.0)
    q = bf16(qb, c.dev)
    for layer in range(c.g.L):
        outs = [mixedgemm.paged_decode(q, d, p, *tbl, layer, 64, window=window) for d, p, tbl in c.both()]
        same(outs, f"paged_decode, layer {layer}, window {window}")
        if window is None:
            hd, hp = c.dequantized_twin()
            want = ko.attention(qb, hd, hp, *c.tables(near=True), layer)
            t_dec.check_attention(outs[1], want, c.v_max(hd, hp, layer))


def test_paged_decode_shared(case):
    c = filled(case)
    qb = rows(np.random.default_rng(4), 2, HQ, 2.0)
    q = bf16(qb, c.dev)
    groups = [i32(a, c.dev) for a in ([0, 2, 2], [0, 1], [c.shared, c.shared])]
    assert c.seq_pages[0][: c.shared // c.g.P] == c.seq_pages[1][: c.shared // c.g.P]
    for layer in range(c.g.L):
        outs = [mixedgemm.paged_decode_shared(q, d, p, *tbl, layer, *groups, c.shared, 64) for d, p, tbl in c.both()]
        same(outs, f"paged_decode_shared, layer {layer}")
        hd, hp = c.dequantized_twin()
        want = ko.attention(qb, hd, hp, *c.tables(near=True), layer)
        t_dec.check_attention(outs[1], want, c.v_max(hd, hp, layer))


@pytest.mark.parametrize("tree", [False, True], ids=["causal", "tree"])
def test_paged_prefill(case, tree):
    c = filled(case)
    T = sum(c.new)
    rng = np.random.default_rng(5)
    qb = rows(rng, T, HQ, 2.0)
    q, qo = bf16(qb, c.dev), np.concatenate([[0], np.cumsum(c.new)]).astype(np.int32)
    words = None
    if tree:                                     # token j attends itself, slot 0 and a random subset of the slots between
        words = np.array([(1 << j) | 1 | (int(rng.integers(0, 1 << 62)) & ((1 << j) - 1)) for n in c.new for j in range(n)], dtype=np.int64)
    for layer in range(c.g.L):
        outs = [mixedgemm.paged_prefill(q, d, p, *tbl, i32(qo, c.dev), layer, 64,
                                        tree_mask=None if words is None else torch.from_numpy(words).to(c.dev)) for d, p, tbl in c.both()]
        same(outs, f"paged_prefill, layer {layer}, tree {tree}")
        if not tree:
            hd, hp = c.dequantized_twin()
            tbl = c.tables(near=True)
            t_pre.check(outs[1], kpo.attention(qb, hd, hp, *tbl, qo, layer), kpo.vmax(qb.shape, hd, hp, *tbl, qo, layer), f"layer {layer}")


def neighbours(c):
    """the pool pages next to a named page that no case names: never written, so they must keep whatever they hold"""
    around = sorted({p + d for p in c.named for d in (-1, 1)} - set(c.named))
    return torch.tensor([p for p in around if 0 <= p < c.g.max_pages], device=c.dev)


def snapshot(c, sel):
    return [raw(t[sel]) for t in (c.data, c.param) if t is not None]


def test_kv_copy_pages(case):
    c = filled(case)
    p0, p31, p32, last, p1 = c.g.pages()
    near_free, far_free_a, far_free_b = c.g.spare_pages()
    pairs = [(p32, near_free, c.g.P), (p1, far_free_a, 5), (last, far_free_b, 9)]             # far -> near, near -> far, far -> far
    assert near_free * c.g.page_bytes < fc.B31 <= min(far_free_a, far_free_b) * c.g.page_bytes
    sel = neighbours(c)
    before = snapshot(c, sel)
    want_d, want_p = c.host_twin()
    for src, dst, n in pairs:
        for w in (want_d, want_p):
            if w is not None:
                w[c.near[dst], :, :, :, :n] = w[c.near[src], :, :, :, :n]
    for (data, param, _), near in zip(c.both(), (False, True)):
        m = (lambda p: c.near[p]) if near else (lambda p: p)
        mixedgemm.kv_copy_pages(data, param, i32([m(s) for s, _, _ in pairs], c.dev), i32([m(d) for _, d, _ in pairs], c.dev),
                                i32([n for _, _, n in pairs], c.dev))
    torch.cuda.synchronize()
    c.assert_far_equals_twin("kv_copy_pages")
    c.assert_twin_is(want_d, want_p, "kv_copy_pages")
    assert all(np.array_equal(a, b) for a, b in zip(before, snapshot(c, sel))), "kv_copy_pages wrote a page next to a named one"


def test_kv_move_rows(case):
    c = filled(case)
    P = c.g.P
    src, dst = [50, 40, 3], [5, 33, 49]            # sequence 0: first past B31 -> first past B32, within the last page, and back
    pages = c.seq_pages[0]
    assert [pages[s // P] for s in src] == [pages[3], pages[2], pages[0]] and [pages[d // P] for d in dst] == [pages[0], pages[2], pages[3]]
    sel = neighbours(c)
    before = snapshot(c, sel)
    want_d, want_p = c.host_twin()
    for w in (want_d, want_p):
        if w is not None:
            moved = [w[c.near[pages[s // P]], :, :, :, s % P].copy() for s in src]
            for d, m in zip(dst, moved):
                w[c.near[pages[d // P]], :, :, :, d % P] = m
    for data, param, tbl in c.both((0,)):
        mixedgemm.kv_move_rows(data, param, tbl[0], tbl[1], i32([0, len(src)], c.dev), i32(src, c.dev), i32(dst, c.dev))
    torch.cuda.synchronize()
    c.assert_far_equals_twin("kv_move_rows")
    c.assert_twin_is(want_d, want_p, "kv_move_rows")
    assert all(np.array_equal(a, b) for a, b in zip(before, snapshot(c, sel))), "kv_move_rows wrote a page next to a named one"
