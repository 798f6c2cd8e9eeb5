"""GPU tests of mixedgemm.logprob_rows and mixedgemm.cross_entropy.  The reference is tests/logprob_oracle.py: the rule in fp64, the
integer outputs from the bf16 bits alone, and the derived bound B on the values; mixedgemm.argmax_rows for column 0 of top_idx and
torch's fp32 cross_entropy on the CPU for the loss.

Every case runs over LAYOUTS: vocab in {1, 7, 8, 9, 255, C - 1, C, C + 1, 2 C + 5} (C = MM_ARGMAX_CHUNK), each at ld = vocab + 3 and
vocab + 4 and at pointer offsets 0 .. 7, 1 .. 5 rows in turn, NaN everywhere outside the rows and a 0xFF-filled workspace.

1 places    n in {1, 2, 3, 8, 1000} columns at one finite value, -inf elsewhere, planted at the first and last columns and +-1 around
            every multiple of 2 048 (so of C): logprob = fl32(-ln n) and lse = fl32(v / T + ln n) within one fp32 ulp, exact for
            n = 1; a -inf target gives -inf and rank n, a planted one rank 0; top_idx the planted columns, then the lowest others
2 integers  rows of random bf16 bits with heavy ties, both zeros, NaNs of both signs, +-inf: rank and top_idx for top_n in
            {1, 2, 5, 20, 32} equal the oracle, column 0 equals argmax_rows, top_n > vocab pads with -1 / -inf
3 values    Gaussian rows (vocab 32 000 and 2 C + 5, 16 rows, temperatures that all differ; one row of 128 256 and of 152 064): every
            logprob, lse and top_logprob within B, no share exempt
4 edges     degenerate rows give NaN with the oracle's integers; ignored targets give 0.0 and -1; T in {0, -1, NaN} is the null T
5 graphs    two calls are bit-equal; one hipGraph replayed after rewriting targets, temperature and logits equals the eager call
6 loss      cross_entropy against torch's on the CPU, three reductions, ignored labels

No bound here comes from what a kernel produced."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from micromix_amd import _lib, mixedgemm
import logprob_oracle as lo
import sample_oracle as so

pytestmark = pytest.mark.gpu

C = _lib.MM_ARGMAX_CHUNK
NINF, NAN_BITS = 0xFF80, 0x7FC0
VOCABS = [1, 7, 8, 9, 255, C - 1, C, C + 1, 2 * C + 5]
LAYOUTS = [(vocab, vocab + 3 + k % 2, k // 2, 1 + (i * 16 + k) % 5) for i, vocab in enumerate(VOCABS) for k in range(16)]

f32 = lambda a, dev: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
i32 = lambda a, dev: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def test_the_layouts_cover_what_they_claim():
    assert {(v, ld - v, off) for v, ld, off, _ in LAYOUTS} == {(v, d, off) for v in VOCABS for d in (3, 4) for off in range(8)}
    assert all({rows for v, _, _, rows in LAYOUTS if v == vocab} == {1, 2, 3, 4, 5} for vocab in VOCABS)


def place(bits, ld, offset, dev):
    """bits [rows, vocab] as a bf16 device view at element `offset` of its allocation, rows ld apart, NaN everywhere else"""
    rows, vocab = bits.shape
    buf = np.full(offset + rows * ld + 16, NAN_BITS, dtype=np.uint16)
    buf[offset: offset + rows * ld].reshape(rows, ld)[:, :vocab] = bits
    t = torch.from_numpy(buf.view(np.int16)).to(dev).view(torch.bfloat16)
    view = t[offset: offset + rows * ld].view(rows, ld)[:, :vocab]
    assert view.data_ptr() == t.data_ptr() + 2 * offset and t.data_ptr() % 16 == 0
    return view


def poisoned_ws(rows, vocab, top_n, dev, fill=0xFF):
    return torch.full((mixedgemm.logprob_rows_workspace_bytes(rows, vocab, top_n),), fill, dtype=torch.uint8, device=dev)


def run(dev, bits, ld=None, offset=0, target=None, T=None, top_n=0, fill=0xFF):
    rows, vocab = bits.shape
    x = place(bits, vocab if ld is None else ld, offset, dev)
    out = mixedgemm.logprob_rows(x, None if target is None else i32(target, dev), temperature=None if T is None else f32(T, dev), top_n=top_n,
                                 workspace=poisoned_ws(rows, vocab, top_n, dev, fill))
    torch.cuda.synchronize()
    assert out.lse.dtype is torch.float32 and tuple(out.lse.shape) == (rows,)
    if target is not None:
        assert out.logprob.dtype is torch.float32 and out.rank.dtype is torch.int32 and tuple(out.rank.shape) == (rows,)
    else:
        assert out.logprob is None and out.rank is None
    if top_n:
        assert out.top_idx.dtype is torch.int32 and tuple(out.top_idx.shape) == tuple(out.top_logprob.shape) == (rows, top_n)
    else:
        assert out.top_idx is None and out.top_logprob is None
    return x, type(out)(*(None if o is None else o.cpu().numpy() for o in out))


def within_one_ulp(got, want):
    got = np.float32(got)
    return abs(float(got) - want) <= float(np.spacing(np.abs(np.float32(want))))


# ---- 1. exact places -------------------------------------------------------------------------------------------------------------------------
def edge_columns(vocab):
    cols = {0, vocab - 1}
    for m in range(0, vocab + 2, 2048):
        cols |= {m - 1, m, m + 1}
    return sorted(c for c in cols if 0 <= c < vocab)


def test_planted_columns_give_exact_answers(dev):
    values, temps = [4.0, -2.5, 100.0, 0.0, -0.0078125], [1.0, 0.5, 1.0, 3.0, 0.7]
    turn = 0
    for vocab, ld, offset, rows in LAYOUTS:
        edges = edge_columns(vocab)
        for n in (1, 2, 3, 8, 1000):
            if n > vocab:
                continue
            bits = np.full((rows, vocab), NINF, dtype=np.uint16)
            planted, target, T = [], [], []
            for r in range(rows):
                turn += 1
                chosen = {edges[(turn * n + j) % len(edges)] for j in range(min(n, len(edges)))}
                for c in range(vocab):                                              # filled up with the lowest other columns
                    if len(chosen) == n:
                        break
                    chosen.add(c)
                cols = sorted(chosen)
                assert len(cols) == n
                bits[r, cols] = so.bf16_bits(np.float32(values[r]))
                others = [c for c in range(min(vocab, n + 40)) if c not in chosen]
                planted.append((cols, others))
                target.append(others[0] if turn % 3 == 0 and others else cols[turn % n])
                T.append(temps[(r + turn) % 5])
            top_n = 12
            _, out = run(dev, bits, ld, offset, target, T, top_n)
            for r, (cols, others) in enumerate(planted):
                where = f"vocab {vocab} ld {ld} offset {offset} rows {rows} n {n} row {r}"
                v, Tr = float(np.float32(values[r])), float(np.float32(T[r]))
                if n == 1:
                    assert out.lse[r] == np.float32(v / Tr) if Tr != 1.0 else out.lse[r] == v, where
                assert within_one_ulp(out.lse[r], v / Tr + math.log(n)), (where, out.lse[r])
                if target[r] in cols:
                    assert out.rank[r] == 0 and within_one_ulp(out.logprob[r], -math.log(n)), (where, out.rank[r], out.logprob[r])
                    assert n > 1 or (out.logprob[r] == 0.0 and not np.signbit(out.logprob[r])), where
                else:
                    assert out.rank[r] == n and out.logprob[r] == -np.inf, (where, out.rank[r], out.logprob[r])
                want = (cols + others)[:top_n]
                want += [-1] * (top_n - len(want))
                assert out.top_idx[r].tolist() == want, (where, out.top_idx[r].tolist(), want)
                for j, c in enumerate(want):
                    if c in cols:
                        assert within_one_ulp(out.top_logprob[r, j], -math.log(n)) and (n > 1 or out.top_logprob[r, j] == 0.0), (where, j)
                    else:
                        assert out.top_logprob[r, j] == -np.inf, (where, j)


# ---- 2. integers, no tolerance ---------------------------------------------------------------------------------------------------------------
def test_rank_and_top_idx_equal_the_oracle_on_rows_with_ties(dev):
    rng = np.random.default_rng(21)
    for case, (vocab, ld, offset, rows) in enumerate(LAYOUTS):
        bits = lo.random_bits(rows, vocab, 500 + case)
        if case % 2:
            bits = np.roll(bits, 1, axis=0)                                         # every kind of row at every row count
        target = rng.integers(0, vocab, rows)
        target[rng.random(rows) < 0.2] = -1
        x = place(bits, ld, offset, dev)
        greedy = mixedgemm.argmax_rows(x).cpu().numpy()
        for top_n in (1, 2, 5, 20, 32):
            where = f"vocab {vocab} ld {ld} offset {offset} rows {rows} top_n {top_n}"
            _, out = run(dev, bits, ld, offset, target, None, top_n)
            for r in range(rows):
                rank, top = lo.integers(bits[r], int(target[r]), top_n)
                assert out.rank[r] == rank, (where, r, out.rank[r], rank)
                assert out.top_idx[r].tolist() == top.tolist(), (where, r, out.top_idx[r].tolist(), top.tolist())
                beyond = top < 0
                assert np.isneginf(out.top_logprob[r][beyond]).all() and beyond.sum() == max(0, top_n - vocab), (where, r)
                if rank < 0:
                    assert out.logprob[r] == 0.0, (where, r)
            assert np.array_equal(out.top_idx[:, 0], greedy), where


# ---- 3. values within the derived bound ------------------------------------------------------------------------------------------------------
def check_rows(out, expected, where):
    bad = []
    for r, (want, e_s) in enumerate(expected):
        assert 0 < e_s <= lo.E_OVER_S_CAP
        assert out.rank[r] == want["rank"] and out.top_idx[r].tolist() == want["top_idx"].tolist(), (where, r)
        pairs = [("logprob", out.logprob[r], want["logprob"]), ("lse", out.lse[r], want["lse"])]
        pairs += [(f"top_logprob[{j}]", g, w) for j, (g, w) in enumerate(zip(out.top_logprob[r], want["top_logprob"]))]
        for name, g, w in pairs:
            msg = lo.check_value(g, w, e_s)
            if msg:
                bad.append((r, name, msg))
    worst = max(abs(float(out.logprob[r]) - e[0]["logprob"]) for r, e in enumerate(expected))
    print(f"{where}: largest logprob error {worst:.3e}, E / S up to {max(e for _, e in expected):.3e}")
    assert not bad, (where, bad[:6])


@pytest.mark.parametrize("vocab", [32000, 2 * C + 5])
def test_gaussian_rows_are_within_the_bound(dev, vocab):
    bits, T, target = lo.gaussian_case(vocab)
    _, out = run(dev, bits, vocab + 3, 1, target, T, lo.TOP_N)
    check_rows(out, lo.gaussian_expected(vocab), f"vocab {vocab}")


@pytest.mark.parametrize("vocab", [128256, 152064])
def test_one_long_row_is_within_the_bound(dev, vocab):
    bits, T, target = lo.long_row(vocab)
    _, out = run(dev, bits, None, 0, target, T, lo.TOP_N)
    check_rows(out, lo.gaussian_expected(vocab, 1), f"vocab {vocab}")


# ---- 4. edges --------------------------------------------------------------------------------------------------------------------------------
def test_degenerate_rows_give_nan_with_the_oracle_integers(dev):
    for vocab, ld, offset, _ in LAYOUTS[::3]:
        rng = np.random.default_rng(vocab)
        bits = so.bf16_bits(np.round(rng.standard_normal((6, vocab)) * 2.0))
        bits[0, vocab // 2] = NAN_BITS
        bits[1, vocab - 1] = 0x7F80                                                 # +inf
        bits[2, :] = NINF                                                           # only -inf
        bits[3, 0] = 0xFFC0                                                         # -NaN
        bits[4, [0, vocab - 1]] = 0x7F80, NAN_BITS                                  # +inf below a NaN
        target = rng.integers(0, vocab, 6)
        _, out = run(dev, bits, ld, offset, target, [1.0, 0.5, 2.0, 1.0, 0.0, 1.0], 3)
        where = f"vocab {vocab} ld {ld} offset {offset}"
        for r in range(6):
            want = lo.row(bits[r], int(target[r]), None, 3)
            assert out.rank[r] == want["rank"] and out.top_idx[r].tolist() == want["top_idx"].tolist(), (where, r)
            if r < 5:
                assert math.isnan(want["lse"]) and np.isnan(out.lse[r]) and np.isnan(out.logprob[r]), (where, r)
                assert np.isnan(out.top_logprob[r][want["top_idx"] >= 0]).all(), (where, r)
                assert np.isneginf(out.top_logprob[r][want["top_idx"] < 0]).all(), (where, r)
            else:
                assert np.isfinite(out.lse[r]) and lo.check_value(out.lse[r], want["lse"], lo.e_over_s(bits[r])) is None, (where, r)


def test_ignored_targets_and_greedy_temperatures(dev):
    for vocab, ld, offset, _ in LAYOUTS[1::3]:
        rng = np.random.default_rng(vocab + 1)
        bits = so.bf16_bits(rng.standard_normal((5, vocab)) * 3.0)
        where = f"vocab {vocab} ld {ld} offset {offset}"
        target = np.array([-100, -1, vocab, 2 ** 31 - 1, vocab - 1], dtype=np.int64)
        x, out = run(dev, bits, ld, offset, target.astype(np.int32), None, 2)
        assert out.logprob[:4].tolist() == [0.0] * 4 and not np.signbit(out.logprob[:4]).any() and out.rank[:4].tolist() == [-1] * 4, where
        assert out.rank[4] == lo.integers(bits[4], vocab - 1, 0)[0], where
        # int64 targets are narrowed on the device, out-of-range values ignored
        wide = torch.from_numpy(np.array([-100, 2 ** 40, -2 ** 40, vocab, vocab - 1], dtype=np.int64)).to(dev)
        o64 = mixedgemm.logprob_rows(x, wide)
        assert o64.rank.tolist() == out.rank.tolist() and o64.logprob.tolist() == out.logprob.tolist(), where
        # T = 0, T < 0, -0 and NaN report the unscaled distribution: the bits of the call without a temperature
        for T in (0.0, -1.0, -0.0, math.nan, -math.inf):
            _, o = run(dev, bits, ld, offset, target.astype(np.int32), [T] * 5, 2)
            for a, b in zip(o, out):
                assert np.array_equal(a.view(np.int32), b.view(np.int32)), (where, T)
        _, scaled = run(dev, bits, ld, offset, target.astype(np.int32), [2.0] * 5, 2)
        assert vocab == 1 or not np.array_equal(scaled.lse, out.lse), where


# ---- 5. determinism and graphs ---------------------------------------------------------------------------------------------------------------
def test_two_calls_are_bit_equal_and_a_graph_replays_rewritten_inputs(dev):
    rows, vocab, top_n = 5, 2 * C + 5, 20
    rng = np.random.default_rng(77)
    fresh = lambda: (so.bf16_bits(rng.standard_normal((rows, vocab)) * 3.0), rng.integers(-1, vocab, rows).astype(np.int32),
                     (0.5 + rng.random(rows)).astype(np.float32))
    bits, tgt, T = fresh()
    a = run(dev, bits, vocab + 3, 3, tgt, T, top_n, fill=0xFF)[1]
    b = run(dev, bits, vocab + 3, 3, tgt, T, top_n, fill=0x00)[1]
    for p, q in zip(a, b):
        assert np.array_equal(p.view(np.int32), q.view(np.int32))
    x = place(bits, vocab + 3, 3, dev)
    target, temp, ws = i32(tgt, dev), f32(T, dev), poisoned_ws(rows, vocab, top_n, dev)
    call = lambda: mixedgemm.logprob_rows(x, target, temperature=temp, top_n=top_n, workspace=ws)
    call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
        with pytest.raises(RuntimeError, match="during graph capture"):
            mixedgemm.logprob_rows(x, target, temperature=0.7, workspace=ws)
    for _ in range(2):
        bits, tgt, T = fresh()
        x.copy_(place(bits, vocab, 0, dev)), target.copy_(i32(tgt, dev)), temp.copy_(f32(T, dev))
        graph.replay()
        torch.cuda.synchronize()
        eager = call()
        for p, q in zip(out, eager):
            assert torch.equal(p.view(torch.int32), q.view(torch.int32)), "the replay and the eager call on the same inputs"
        want = lo.row(bits[0], int(tgt[0]), T[0], top_n)
        assert out.top_idx[0].tolist() == want["top_idx"].tolist() and out.rank[0].item() == want["rank"]


# ---- 6. cross_entropy ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab", [1000, 2 * C + 5])
def test_cross_entropy_equals_torch_on_the_cpu(dev, vocab):
    rows = 33
    rng = np.random.default_rng(vocab)
    bits = so.bf16_bits(rng.standard_normal((rows, vocab)) * 3.0)
    labels = rng.integers(0, vocab, rows)
    labels[[2, 17, 32]] = -100
    x, y = place(bits, vocab + 3, 1, dev), torch.from_numpy(labels).to(dev)
    ref_x, ref_y = x.float().cpu(), y.cpu()
    B = max(lo.bound(lo.e_over_s(bits[r]), lo.row(bits[r], int(labels[r]))["logprob"]) for r in range(rows) if labels[r] >= 0)
    for reduction in ("mean", "sum", "none"):
        got = mixedgemm.cross_entropy(x, y, reduction=reduction)
        want = F.cross_entropy(ref_x, ref_y, reduction=reduction)
        assert got.dtype is torch.float32 and got.shape == want.shape and got.device == x.device
        err = (got.cpu().double() - want.double()).abs()
        tol = B + 2.0 ** -22 * want.double().abs()
        print(f"vocab {vocab} {reduction}: largest error {float(err.max()):.3e}, tolerance there {float(tol.flatten()[err.argmax()]):.3e}")
        assert bool((err <= tol).all()), (reduction, float(err.max()))
    assert mixedgemm.cross_entropy(x, y, reduction="none")[[2, 17, 32]].tolist() == [0.0] * 3
    other = torch.where(y == -100, 5, y)
    assert torch.equal(mixedgemm.cross_entropy(x, other, ignore_index=5), mixedgemm.cross_entropy(x, torch.where(y == 5, -100, y)))
    assert torch.equal(mixedgemm.cross_entropy(x, y.to(torch.int32)), mixedgemm.cross_entropy(x, y))


def test_python_argument_errors_on_the_device(dev):
    x = torch.zeros((3, 100), dtype=torch.bfloat16, device=dev)
    y = torch.zeros((3,), dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="top_n"):
        mixedgemm.logprob_rows(x, top_n=33)
    with pytest.raises(ValueError, match="top_n"):
        mixedgemm.logprob_rows(x, top_n=-1)
    with pytest.raises(RuntimeError, match="targets must be"):
        mixedgemm.logprob_rows(x, y[:2])
    with pytest.raises(TypeError, match="targets"):
        mixedgemm.logprob_rows(x, [0, 1, 2])
    with pytest.raises(TypeError, match="int32"):
        mixedgemm.logprob_rows(x, y.float())
    with pytest.raises(TypeError, match="temperature must be None, a number"):
        mixedgemm.logprob_rows(x, y, temperature="hot")
    with pytest.raises(RuntimeError, match="workspace"):
        mixedgemm.logprob_rows(x, y, workspace=torch.zeros(8, dtype=torch.uint8, device=dev))
    with pytest.raises(TypeError, match="labels"):
        mixedgemm.cross_entropy(x, y.float())
    with pytest.raises(RuntimeError, match="labels must be"):
        mixedgemm.cross_entropy(x, y[:2])
    out = mixedgemm.logprob_rows(x[:0])
    assert tuple(out.lse.shape) == (0,) and mixedgemm.cross_entropy(x[:0], y[:0], reduction="sum").item() == 0.0
