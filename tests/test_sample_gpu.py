"""GPU tests of mixedgemm.sample_rows.  The references are tests/sample_oracle.py (the rule in fp64 and the admissible set its derived
bound allows), mixedgemm.argmax_rows for the greedy cases and a twin cache that runs accept(oracle paths) for the captured step.

1 places   every row holds n columns at one finite value and -inf (even rows) or a value about 1000 lower (odd rows) elsewhere, so the
           weights are 1 and 0, the CDF is integers and u = (j + 0.5) / n must return the j-th planted column: every column of the
           first and last 300, +-9 around every multiple of MM_ARGMAX_CHUNK, +-1 around every multiple of 2 048 at vocab = 2 CHUNK + 5
           with ld = vocab + 3 and vocab + 4, eight small vocabularies, pointer offsets 0 .. 7; NaN everywhere outside the rows, a
           NaN-filled workspace; without filters and with top-k = n, top-p = 0.999 and min-p = 0.5, which keep exactly the planted class
2 filters  three classes of 3, 5 and 1 000 tokens, the third at the highest indices, drawn with u = 1 - 2^-24 (tests/sample_cases.py;
           tests/test_sample_cpu.py proves every decision has a margin of 1e-3): top-k with ties, top-p, min-p, all three with each
           binding in turn, off values of every parameter, classes in one level-1 bin and in three, negative values, +0 with -0,
           T in {0.5, 1, 2}, one and three parts; with per-row arrays, and with Python numbers for one row
3 greedy   T = 0, T < 0, T = NaN, rows holding a NaN, +inf or only -inf equal argmax_rows bit for bit
4 sets     Gaussian rows (vocab 32 000 and 2 CHUNK + 5, 64 rows, parameters that all differ), a 1 000-token row repeated 4 096 times
           with stratified u, single rows of 128 256 and 152 064: every row returns an admissible token, no share exempt
5 graph    two calls are bit-equal; one hipGraph of sample_rows -> verify_launch replayed after rewriting u, T, top_k and the tree
6 errors   the Python argument errors that need a device tensor to be reached; no rows

No bound here comes from what a kernel produced."""
import numpy as np
import pytest
import torch

from micromix_amd import _lib, mixedgemm
from micromix_amd.kvcache import PagedKVCache
import kv_verify_oracle as kvo
import sample_cases as sc
import sample_oracle as so
import test_kv_tree_gpu as t_tree
import test_kv_verify_gpu as t_ver

pytestmark = pytest.mark.gpu

C = _lib.MM_ARGMAX_CHUNK
NAN = float("nan")
i32 = t_tree.i32
f32 = lambda a, dev: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def poisoned_ws(rows, vocab, dev):
    return torch.full((mixedgemm.sample_rows_workspace_bytes(rows, vocab),), 0xFF, dtype=torch.uint8, device=dev)


def from_bits(bits, dev, ld=None):
    """bf16 [rows, vocab] on the device, the columns behind vocab (up to ld) NaN"""
    rows, vocab = bits.shape
    full = np.full((rows, vocab if ld is None else ld), 0x7FC0, dtype=np.uint16)
    full[:, :vocab] = bits
    return torch.from_numpy(full.view(np.int16)).to(dev).view(torch.bfloat16)[:, :vocab]


# ---- 1. places ---------------------------------------------------------------------------------------------------------------------------
def test_exp2_of_zero_is_one(dev):
    """what makes the CDF of an all-equal row integers: the maximum's weight is exactly 1 -- two equal tokens split u at 1/2 exactly"""
    x = torch.full((2, 2), 3.0, dtype=torch.bfloat16, device=dev)
    u = f32([0.5 - 2.0 ** -25, 0.5], dev)
    assert mixedgemm.sample_rows(x, u, temperature=f32([0.37, 1.9], dev)).tolist() == [0, 1]


def check_places(dev, vocab, ld, offset):
    cols = sc.chosen_columns(vocab) if vocab > 300 else list(range(vocab))
    n = len(cols)
    buf = torch.full((offset + n * ld + 16,), NAN, dtype=torch.bfloat16, device=dev)
    view = buf[offset: offset + n * ld].view(n, ld)[:, :vocab]
    view[0::2] = float("-inf")
    view[1::2] = -992.0                                      # about 1000 below the planted value, a bf16: weight 0
    view[:, torch.tensor(cols, dtype=torch.int64, device=dev)] = 4.0
    assert view.data_ptr() % 16 == (buf.data_ptr() + 2 * offset) % 16 and (view.stride(0) == ld or n == 1)
    u = f32((np.arange(n) + 0.5) / n, dev)
    want = np.array(cols)
    for filtered in (False, True):
        kw = dict(top_k=i32([n] * n, dev), top_p=f32([0.999] * n, dev), min_p=f32([0.5] * n, dev)) if filtered else {}
        got = mixedgemm.sample_rows(view, u, workspace=poisoned_ws(n, vocab, dev), **kw)
        torch.cuda.synchronize()
        assert got.dtype == torch.int32 and tuple(got.shape) == (n,)
        got = got.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert not len(bad), (f"vocab {vocab} ld {ld} offset {offset} filters {filtered}: {len(bad)} of {n} rows wrong, first row "
                              f"{bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}")


@pytest.mark.parametrize("offset", range(8))
def test_every_planted_column_is_drawn_by_its_u(dev, offset):
    vocab = 2 * C + 5
    check_places(dev, vocab, vocab + 3, offset)
    check_places(dev, vocab, vocab + 4, offset)              # an odd row distance: the rows of one call start at every alignment
    for small in (1, 7, 8, 9, 255, 257, C - 1, C + 1):
        check_places(dev, small, small, offset)


# ---- 2. filters with an exact answer ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(len(sc.TRIPLES)), ids=[t[0] for t in sc.TRIPLES])
def test_filters_with_an_exact_answer(dev, which):
    bits, T, rows, last = sc.filter_case(which)
    n, vocab = len(rows), len(bits)
    x = from_bits(np.tile(bits, (n, 1)), dev, ld=vocab + 3)
    want = [last[r[4] - 1] for r in rows]
    u = f32([sc.U_LAST] * n, dev)
    par = dict(temperature=f32([T] * n, dev), top_k=i32([r[1] for r in rows], dev), top_p=f32([r[2] for r in rows], dev),
               min_p=f32([r[3] for r in rows], dev))
    got = mixedgemm.sample_rows(x, u, workspace=poisoned_ws(n, vocab, dev), **par).tolist()
    assert got == want, [(r[0], g, w) for r, g, w in zip(rows, got, want) if g != w]
    # null arrays are filters that are off; Python numbers are broadcast
    for r, (label, k, p, q, _) in enumerate(rows[:12]):
        one = mixedgemm.sample_rows(x[r:r + 1], u[:1], temperature=T, top_k=k or None, top_p=None if p == 1.0 else p,
                                    min_p=q or None).tolist()
        assert one == [want[r]], label
    # u = 0 draws the first kept token whatever the filters: the first token of the first class
    first = mixedgemm.sample_rows(x, torch.zeros_like(u), **par).tolist()
    assert first == [min(7, 3) if r[4] > 1 else 7 for r in rows]


# ---- 3. greedy equality ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab", [97, 2 * C + 5])
def test_greedy_cases_equal_argmax_rows(dev, vocab):
    rng = np.random.default_rng(vocab)
    bits = so.bf16_bits(np.round(rng.standard_normal((12, vocab)) * 2.0))            # ties everywhere: the lowest index must win
    bits[3, vocab - 2] = 0x7FC0                              # NaN
    bits[4, vocab // 2] = 0x7F80                             # +inf
    bits[5, :] = 0xFF80                                      # only -inf
    bits[6, 1] = 0xFFC0                                      # -NaN
    bits[7, [2, vocab - 1]] = 0x7F80                         # +inf twice
    T = np.array([0.0, -1.0, NAN, 1.0, 1.0, 1.0, 1.0, 0.7, -0.0, 0.0, NAN, float("-inf")], dtype=np.float32)
    for r in range(12):
        assert so.is_greedy(bits[r], T[r]), r
    x = from_bits(bits, dev, ld=vocab + 1)
    want = mixedgemm.argmax_rows(x)
    got = mixedgemm.sample_rows(x, f32([0.99] * 12, dev), temperature=f32(T, dev), top_k=i32([5] * 12, dev), top_p=f32([0.5] * 12, dev),
                                min_p=f32([0.1] * 12, dev), workspace=poisoned_ws(12, vocab, dev))
    assert torch.equal(got, want) and want.tolist() == kvo.argmax_rows(bits).tolist()
    assert torch.equal(mixedgemm.sample_rows(x, f32([0.99] * 12, dev), temperature=f32(T, dev)), want)


# ---- 4. the admissible set on realistic rows -------------------------------------------------------------------------------------------------
def run_rows(dev, bits, par):
    x = from_bits(bits, dev)
    out = mixedgemm.sample_rows(x, f32(par["u"], dev), temperature=f32(par["T"], dev), top_k=i32(par["k"], dev), top_p=f32(par["p"], dev),
                                min_p=f32(par["q"], dev), workspace=poisoned_ws(*bits.shape, dev))
    torch.cuda.synchronize()
    return x, out


@pytest.mark.parametrize("vocab", [32000, 2 * C + 5])
def test_gaussian_rows_return_admissible_tokens(dev, vocab):
    bits, par = so.gaussian_case(vocab, so.GAUSSIAN_ROWS, vocab)
    sets = so.gaussian_admissible(vocab)
    x, out = run_rows(dev, bits, par)
    got = out.tolist()
    print(f"vocab {vocab}: {sum(len(s) > 1 for s in sets)} of {len(sets)} rows with more than one admissible token")
    bad = [(r, g, sorted(s)[:4]) for r, (g, s) in enumerate(zip(got, sets)) if g not in s]
    assert not bad, bad[:8]
    # the same call again, over another workspace: the same bits
    again = mixedgemm.sample_rows(x, f32(par["u"], dev), temperature=f32(par["T"], dev), top_k=i32(par["k"], dev), top_p=f32(par["p"], dev),
                                  min_p=f32(par["q"], dev), workspace=torch.zeros_like(poisoned_ws(*bits.shape, dev)))
    assert torch.equal(out, again)


def test_stratified_draws_follow_the_cdf(dev):
    bits, u, p = so.stratified_case()
    n = so.STRATIFIED_ROWS
    sets = so.stratified_admissible()
    par = dict(u=u, T=[p["T"]] * n, k=[p["k"]] * n, p=[p["p"]] * n, q=[0.0] * n)
    _, out = run_rows(dev, np.tile(bits, (n, 1)), par)
    got = out.cpu().numpy()
    print(f"stratified: {sum(len(s) > 1 for s in sets)} of {n} rows with more than one admissible token")
    bad = [(r, int(g)) for r, (g, s) in enumerate(zip(got, sets)) if int(g) not in s]
    assert not bad, bad[:8]
    # the histogram of the outputs against the fp64 CDF: token i is drawn floor / ceil of 4096 * w_i / Z times, give or take the rows
    # whose admissible set holds it besides another token
    keep = so.kept_mask(bits, p["T"], p["k"], p["p"], None)
    w, _ = so.weights(bits, p["T"])
    share = np.where(keep, w, 0.0) / w[keep].sum() * n
    hist = np.bincount(got, minlength=len(bits))
    slack = np.bincount([i for s in sets if len(s) > 1 for i in s], minlength=len(bits))
    assert (np.abs(hist - share) <= 1.0 + slack).all() and set(np.flatnonzero(hist).tolist()) <= set.union(*sets)


@pytest.mark.parametrize("vocab", [128256, 152064])
def test_one_long_row_returns_the_admissible_token(dev, vocab):
    bits, p = so.long_row(vocab)
    want = so.admissible(bits, p["u"], p["T"], p["k"], p["p"], p["q"])
    _, out = run_rows(dev, bits[None, :], {k: [v] for k, v in p.items()})
    assert out.item() in want, (out.item(), want)
    # the last column and the first, by u, with every filter off
    x = from_bits(bits[None, :], dev)
    ends = mixedgemm.sample_rows(x.expand(2, vocab).contiguous(), f32([0.0, 1.0], dev)).tolist()
    assert ends[0] in so.admissible(bits, 0.0) and ends[1] in so.admissible(bits, 1.0) and ends[0] < 50 and ends[1] > vocab - 50


# ---- 5. one graph: sample_rows -> verify_launch ---------------------------------------------------------------------------------------------
def test_graph_of_sample_and_verify_replays_with_other_parameters_and_another_tree(dev):
    B, Hkv, n, V = 2, 2, 12, t_ver.V
    rng = np.random.default_rng(91)
    rnd = lambda m: t_tree.bf(rng.standard_normal((m, Hkv, 128)), dev)
    trees = [[[-1, 0, 0, 1, 1, 2, 2, 3, 4, 5, 6, 7], None], [[-1, -1, 0, 1, 2, 2, 4, 5, 5, 8, 8, 10], [-1] + [0] * 11]]
    chosen = [[[0, 2, 5], [0, 1, 2, 3]], [[1, 3], [0, 7]]]
    prior = [rnd(79), rnd(79)]
    steps = [(rnd(B * n), rnd(B * n)) for _ in trees]
    ours, twin = (PagedKVCache(1, Hkv, 16, 64, B, kind="bf16", device=dev) for _ in range(2))
    for c in (ours, twin):
        c.extend([70, 9])
        c.append(0, *prior)
    T = B * n
    logits = torch.zeros((T, V), dtype=torch.bfloat16, device=dev)
    draft, root, target = i32([0] * T, dev), i32([-1] * B, dev), i32([0] * T, dev)
    u, temp, top_k = f32([0.5] * T, dev), f32([1.0] * T, dev), i32([0] * T, dev)
    top_p, min_p = f32([0.95] * T, dev), f32([0.001] * T, dev)
    ws = poisoned_ws(T, V, dev)
    call = lambda out: mixedgemm.sample_rows(logits, u, temperature=temp, top_k=top_k, top_p=top_p, min_p=min_p, out=out, workspace=ws)
    ours.extend(n)
    ours.tree_mask(trees[0])
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call(target)
        result = ours.verify_launch(target, draft, root)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert result[:, 0].tolist() == [n, n]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(target)
        assert ours.verify_launch(target, draft, root) is result
        with pytest.raises(RuntimeError, match="during graph capture"):
            mixedgemm.sample_rows(logits, u, temperature=0.7, out=target, workspace=ws)
    for step, (tree, paths) in enumerate(zip(trees, chosen)):
        # a path's rows carry 60 in the wanted column: weight 1 against e^-50, so every u and every filter draws it; the other rows
        # are Gaussian and their draws move with u, T and top_k
        d, r, lg = t_ver.draft_step(rng, [n, n], paths, dev)
        for c in (ours, twin):
            if step or c is twin:
                c.extend(n)
            mask = c.tree_mask(tree)[0]
            c.append(0, *steps[step])
        draft.copy_(d), root.copy_(r), logits.copy_(lg)
        u.copy_(f32(rng.random(T), dev)), temp.copy_(f32(0.5 + rng.random(T), dev)), top_k.copy_(i32(rng.integers(0, 40, T), dev))
        graph.replay()
        torch.cuda.synchronize()
        eager = call(torch.empty_like(target))
        assert torch.equal(target, eager), "the replay and the eager call on the same inputs"
        got = ours.commit(result)
        want = kvo.verify(eager.cpu().numpy(), d.cpu().numpy(), r.cpu().numpy(), [int(w) for w in mask.tolist()],
                          twin.append_indptr.cpu().numpy(), twin.kv_indptr.cpu().numpy(), twin.last_page_len.cpu().numpy(), 16)
        assert kvo.paths_of(want[0], [n, n]) == paths, "precondition: the logits must make the chosen paths win"
        assert np.array_equal(result.cpu().numpy(), want[0]) and got == (paths, [7, 7])
        twin.accept(paths)
        torch.cuda.synchronize()
        t_ver.same_cache(ours, twin, f"replay {step}")
    assert ours.seq_lens == [70 + 3 + 2, 9 + 4 + 2]
    assert len(set(target.tolist())) > 6, "the rows off the paths must have drawn different tokens"


# ---- 6. Python argument errors that need a device tensor to be reached ------------------------------------------------------------------------
def test_python_argument_errors_on_the_device(dev):
    x = torch.zeros((3, 100), dtype=torch.bfloat16, device=dev)
    u = torch.full((3,), 0.5, device=dev)
    with pytest.raises(TypeError, match="u must be"):
        mixedgemm.sample_rows(x, 0.5)
    with pytest.raises(TypeError, match="float32"):
        mixedgemm.sample_rows(x, u.double())
    with pytest.raises(RuntimeError, match=r"u must be torch.float32 \[3\]"):
        mixedgemm.sample_rows(x, u[:2])
    with pytest.raises(TypeError, match="int32"):
        mixedgemm.sample_rows(x, u, top_k=torch.ones(3, dtype=torch.int64, device=dev))
    with pytest.raises(TypeError, match="top_k must be an int"):
        mixedgemm.sample_rows(x, u, top_k=2.5)
    with pytest.raises(TypeError, match="temperature must be None, a number"):
        mixedgemm.sample_rows(x, u, temperature="hot")
    with pytest.raises(RuntimeError, match="min_p must be a device tensor"):
        mixedgemm.sample_rows(x, u, min_p=torch.zeros(3))                            # a CPU tensor
    with pytest.raises(RuntimeError, match=r"out must be int32 \[3\]"):
        mixedgemm.sample_rows(x, u, out=torch.zeros(4, dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError, match="workspace"):
        mixedgemm.sample_rows(x, u, workspace=torch.zeros(8, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match="unit stride"):
        mixedgemm.sample_rows(x.t()[:100, :3].t()[:, ::2], u)
    # no rows: nothing to do; all equal logits and u = 0.5 of 100: column 50
    assert mixedgemm.sample_rows(x[:0], u[:0]).numel() == 0
    assert mixedgemm.sample_rows(x, u, top_k=100, top_p=1.0, min_p=0).tolist() == [50, 50, 50]
