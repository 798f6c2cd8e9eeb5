"""tests/test_far_kv_gpu.py for the paged cache of 64-wide heads (include/micromix_kv_hd64.h, micromix_kv_prefill_hd64.h): one pool per
kind (bf16, fp8) whose data tensor is just over 4 GiB (far_cases.POOLS_HD64; rows of 128 and 64 bytes), from torch.empty; only the
pages a case names are ever written, and only by the library.  Every page list mixes page 0, the first page wholly past 2^31 bytes, the
first wholly past 2^32 bytes and the last page, and page 1, which is where a 32-bit offset of the last page lands
(tests/test_far_cpu.py).  The headers' "row offsets are 64-bit" and the per-lane 64-bit addresses the prefill hands to its LDS-DMA
are what this runs.

Each case has a twin: the same calls on a cache of nine pages that starts as a copy of the pool's named pages, with the page ids
remapped to 0 .. 8.  The far pages must equal the twin's byte for byte, and q_rot, k_out / v_out and every attention output the twin's
bit for bit; the small cache itself is held to exact answers and to fp64 by the other 64-wide tests."""
import numpy as np
import pytest
import torch

from micromix_amd import mixedgemm
import far_cases as fc

pytestmark = pytest.mark.gpu

HQ = 8
i32 = lambda a, dev: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def bf16(bits, dev):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)


def raw(t):
    return t.detach().contiguous().view(torch.uint8).cpu().numpy()


class Case:
    """the pool of one kind, its twin, and two sequences: sequence 0 on pages [first past B32, 0, last, first past B31] with 57 tokens,
    sequence 1 sharing the first two of them and ending on page 1, 43 tokens"""

    def __init__(self, kind, dev):
        g = self.g = fc.POOLS_HD64[kind]
        self.kind, self.dev = kind, dev
        shape = (g.L, 2, g.Hkv, g.P)
        if kind == "bf16":
            self.data, self.param = torch.empty((g.max_pages,) + shape + (64,), dtype=torch.bfloat16, device=dev), None
        else:
            self.data = torch.empty((g.max_pages,) + shape + (64,), dtype=torch.uint8, device=dev).view(torch.float8_e4m3fn)
            self.param = torch.empty((g.max_pages,) + shape + (2,), dtype=torch.float16, device=dev)
        assert self.data.numel() * self.data.element_size() == g.data_bytes() > fc.B32
        p0, p31, p32, last, p1 = g.pages()
        assert (p0, p1) == (0, 1) and g.far_pages() == [p0, p31, p32, last]
        self.named = g.pages() + g.spare_pages()                                  # twin page i holds pool page named[i]
        assert len(set(self.named)) == len(self.named) == 8 and max(self.named) < g.max_pages
        self.near = {p: i for i, p in enumerate(self.named)}
        sel = torch.tensor(self.named, device=dev)
        u8 = self.data.view(torch.uint8)
        self.twin_data = torch.cat([u8[sel], torch.zeros_like(u8[:1])]).view(self.data.dtype)
        self.twin_param = None if self.param is None else torch.cat([self.param[sel], torch.zeros_like(self.param[:1])])
        self.seq_pages = [[p32, p0, last, p31], [p32, p0, p1]]
        self.lens = [57, 43]
        self.new = [7, 11]                                                        # the tokens of the second append and of the prefill

    def tables(self, seqs=(0, 1), lens=None, near=False):
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

    def assert_far_equals_twin(self, what):
        sel = torch.tensor(self.named, device=self.dev)
        n = len(self.named)
        for name, far, twin in (("data", self.data, self.twin_data), ("param", self.param, self.twin_param)):
            if far is not None:
                a, b = raw(far.view(torch.uint8)[sel] if name == "data" else far[sel]), raw(twin[:n])
                bad = (a != b).reshape(n, -1).any(axis=1)
                assert not bad.any(), f"{what}: {name} of pool pages {[self.named[i] for i in np.flatnonzero(bad)]} differ from the twin's"


@pytest.fixture(scope="module", params=["fp8", "bf16"])
def case(request, dev):
    """one pool at a time"""
    need, free = fc.POOLS_HD64[request.param].need_bytes(), torch.cuda.mem_get_info(dev)[0]
    if free < need:
        pytest.skip(f"the far 64-wide {request.param} pool needs {need / fc.GIB:.1f} GiB of device memory (tests/far_cases.py), "
                    f"{free / fc.GIB:.1f} GiB are free")
    box = [Case(request.param, dev)]
    yield box[0]
    box[0].__dict__.clear()
    box.clear()
    torch.cuda.empty_cache()


def rows(rng, n, heads, scale):
    return fc.bf16_bits(rng.standard_normal((n, heads, 64)) * scale)


def same(outs, what):
    assert torch.equal(outs[0].contiguous().view(torch.int16), outs[1].contiguous().view(torch.int16)), f"{what}: the far pool's output differs from the twin's"


def fill(c, dense):
    """append every token of both sequences to both layers of the pool and of the twin, in two steps (sequence 0's first 50 tokens,
    then 7 and 11 new ones): every page gets its own content; dense: rope_kv_append_dense and its k_out / v_out, else rope_kv_append
    for the first layer and kv_append for the second"""
    rng = np.random.default_rng(len(c.kind) + dense)
    steps = [((0,), [c.lens[0] - c.new[0]], [c.lens[0] - c.new[0]]), ((0, 1), c.lens, c.new)]
    for layer in range(c.g.L):
        for seqs, lens, new in steps:
            T = sum(new)
            q, k, v = (bf16(rows(rng, T, h, s), c.dev) for h, s in ((HQ, 1.0), (c.g.Hkv, 2.0), (c.g.Hkv, 0.5)))
            ang = torch.from_numpy(rng.uniform(0, 6.28, (T, 64)).astype(np.float32))
            cos, sin = ang.cos().to(torch.bfloat16).to(c.dev), ang.sin().to(torch.bfloat16).to(c.dev)
            app = i32(np.concatenate([[0], np.cumsum(new)]), c.dev)
            outs = []
            for data, param, tbl in c.both(seqs, lens):
                if dense:
                    outs.append(mixedgemm.rope_kv_append_dense(data, param, *tbl, q, k, v, cos, sin, app, layer))
                elif layer == 0:
                    outs.append((mixedgemm.rope_kv_append(data, param, *tbl, q, k, v, cos, sin, app, layer),))
                else:
                    mixedgemm.kv_append(data, param, *tbl, k, v, app, layer)
            for far, twin, name in zip(*outs, ("q_rot", "k_out", "v_out")) if outs else ():
                same((far, twin), f"layer {layer}: {name}")
    torch.cuda.synchronize()
    c.assert_far_equals_twin("rope_kv_append_dense" if dense else "rope_kv_append / kv_append")
    c.filled = True


def filled(c):
    if not getattr(c, "filled", False):
        fill(c, dense=False)
    return c


def test_append(case):
    fill(case, dense=False)


def test_append_dense(case):
    fill(case, dense=True)


def test_paged_decode(case):
    c = filled(case)
    q = bf16(rows(np.random.default_rng(3), 2, HQ, 2.0), c.dev)
    for layer in range(c.g.L):
        same([mixedgemm.paged_decode(q, d, p, *tbl, layer, 64) for d, p, tbl in c.both()], f"paged_decode, layer {layer}")


@pytest.mark.parametrize("new", [(40, 30), (1, 1)], ids=["rows128", "rows64"])
def test_paged_prefill(case, new):
    """both workgroup shapes; the bf16 one fetches its rows by LDS-DMA from per-lane 64-bit addresses"""
    c = filled(case)
    T = sum(new)
    assert mixedgemm.paged_prefill_hd64_plan(T, 2, HQ, c.g.Hkv, 64).rows == (128 if T > 2 else 64)
    q, qo = bf16(rows(np.random.default_rng(5), T, HQ, 2.0), c.dev), i32(np.concatenate([[0], np.cumsum(new)]), c.dev)
    for layer in range(c.g.L):
        same([mixedgemm.paged_prefill(q, d, p, *tbl, qo, layer, 64) for d, p, tbl in c.both()], f"paged_prefill, layer {layer}")
