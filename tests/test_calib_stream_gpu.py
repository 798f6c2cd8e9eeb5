"""GPU tests of the streaming calibration (micromix_amd.calib.accumulate / Calibrator over mm_calib_accumulate) against torch on the CPU
(tests/calib_oracle.py).  R = 8 rows form a slice of the kernel (include/micromix_calib.h), so the row counts are
{1, 2, R - 1, R, R + 1, 2 R + 3, 257}; K in {128, 1152, 4096, 32768} takes every instantiation of the row kernel but the 8-piece one,
which K = 14336 adds.

1 exact     integer-valued inputs, |x| <= 256: every partial sum is exact, so score equals fp32(fp64 sum / rows) bit for bit and the
            counts equal torch's, after every batch of a run of seven whose per-channel maximum comes from a different batch per channel
2 edges     planted rows on both sides of exact thresholds, subnormal and infinite thresholds, zero / inf / NaN rows, lamda 1 and 0.7;
            the same in fp16
3 gauss     tests/test_calib.py's input in bf16, batches of 100, 1 and 411 rows: exact counts, score within the header's bound, the order
4 bounds    a slice of a NaN-filled tensor; a misaligned view through the copy
5 state     a 0xFF workspace, two runs, guard elements, no rows
6 hooks     three nn.Linear layers hooked with Calibrator.hook

BOUND is the header's: (R + 1) * 2^-24 relative.  No bound here comes from what the kernel produced."""
import pytest
import torch

from micromix_amd import calib
import calib_oracle as co

pytestmark = pytest.mark.gpu

R = 8
ROWS = (1, 2, R - 1, R, R + 1, 2 * R + 3, 257)
BOUND = (R + 1) * 2.0 ** -24
NAN, INF = float("nan"), float("inf")


def fresh(k, dev, guard=0):
    return torch.zeros(k + guard, dtype=torch.float32, device=dev)[:k], torch.zeros(2 + guard, dtype=torch.int64, device=dev)[:2]


def run(batches, dev, lamda=1.0, **kw):
    """(score, [count4, count6]) on the host after the batches, from the empty state"""
    score, counts = fresh(batches[0].shape[-1], dev)
    for x in batches:
        calib.accumulate(x.to(dev), score, counts, lamda, **kw)
    return score.cpu(), counts.tolist()


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. exact ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("k", [128, 1152, 4096, 14336, 32768])
def test_exact(dev, k, dtype):
    g = torch.Generator().manual_seed(k)
    batches = []
    for i, rows in enumerate(ROWS):
        x = torch.randint(-100, 101, (rows, k), generator=g).float()
        x[:, i::len(ROWS)] += torch.where(x[:, i::len(ROWS)] < 0, -150.0, 150.0)       # batch i holds the maximum of channels i, i + 7, ...
        batches.append(x.to(dtype))
    score, counts = fresh(k, dev)
    for n, x in enumerate(batches):
        calib.accumulate(x.to(dev), score, counts)
        want = co.run(batches[:n + 1])
        assert torch.equal(bits(score.cpu()), bits(want["score"])), (n, x.shape)
        assert counts.tolist() == [want["count4"], want["count6"]], (n, x.shape)
    assert torch.stack(want["means"]).argmax(dim=0)[:len(ROWS)].tolist() == list(range(len(ROWS)))     # channel i's maximum is batch i's
    assert 0 < counts[0] < counts[1] < want["numel"]


# ---- 2. edges ----------------------------------------------------------------------------------------------------------------------------
BF16_MAX = float(torch.tensor(0x7F7F, dtype=torch.int16).view(torch.bfloat16))
# (the row's maximum, the other values planted in it, how many of the planted values lie below t4 and t6 at lamda = 1)
EDGE_ROWS = [
    (96.0, [7.0, 24.0, 6.96875, 23.875, -7.0, -6.96875], (2, 5)),                # t4 = 7, t6 = 24 exactly: 7 and 24 are not below them
    (3.0, [0.21875, 0.2177734375, 0.75, 0.74609375], (1, 3)),                    # t4 = 0.21875, t6 = 0.75
    (3 * 2.0 ** -120, [2.0 ** -123, 2.0 ** -121, 2.0 ** -120], (1, 2)),           # t4 = 0.21875 * 2^-120, t6 = 0.75 * 2^-120
    (3 * 2.0 ** -133, [2.0 ** -133, 2.0 ** -132], (0, 0)),                       # subnormal thresholds: only the zeros lie below
    (BF16_MAX, [1.0], (1, 1)),                                                   # m * 448 overflows: infinite thresholds, m is below too
    (0.0, [], (0, 0)),                                                           # an all-zero row: 0 < 0 is false
    (INF, [5.0, -INF], (1, 1)),                                                  # infinite thresholds, the infinities are not below
    (NAN, [1.0, 2.0], (0, 0)),                                                   # a NaN row counts nothing
]


def edge_batch(k):
    """one planted row each, the rest of a row zero, the planted values of row r at columns 3 r + 11 j; then two Gaussian rows"""
    x = torch.zeros(len(EDGE_ROWS) + 2, k)
    for r, (m, others, _) in enumerate(EDGE_ROWS):
        for j, v in enumerate([m] + others):
            x[r, (3 * r + 11 * j) % k] = v
    x[-2:] = torch.randn(2, k, generator=torch.Generator().manual_seed(1))
    return x.bfloat16()


@pytest.mark.parametrize("k", [128, 1152])
def test_threshold_edges(dev, k):
    x = edge_batch(k)
    for r, (m, others, (n4, n6)) in enumerate(EDGE_ROWS):          # the sides stated above are torch's on the CPU
        v = x[r:r + 1].float().abs()
        assert torch.equal(v.sort().values[0, -1 - len(others):].nan_to_num(-1, -2, -3),
                           torch.tensor([abs(m)] + [abs(o) for o in others]).sort().values.nan_to_num(-1, -2, -3)), r   # bf16 holds them
        t4, t6 = co.thresholds(v)
        free = (int((v == 0).sum()) if m > 0 else 0) + (m == BF16_MAX)       # the zeros lie below every positive threshold
        assert (int((v < t4).sum()), int((v < t6).sum())) == (n4 + free, n6 + free), r
    assert co.thresholds(torch.tensor([[96.0]])) == (7.0, 24.0) and co.thresholds(torch.tensor([[3.0]]))[0] == 0.21875
    assert 0 < co.thresholds(torch.tensor([[3 * 2.0 ** -133]]))[1] < 2.0 ** -126 and co.thresholds(torch.tensor([[BF16_MAX]]))[0] == INF
    for lamda in (1.0, 0.7):
        for r in range(x.shape[0]):                                # every row alone, then the batch
            want = co.run([x[r:r + 1]], lamda)
            assert run([x[r:r + 1]], dev, lamda)[1] == [want["count4"], want["count6"]], (lamda, r)
        want = co.run([x], lamda)
        score, counts = run([x], dev, lamda)
        assert counts == [want["count4"], want["count6"]], lamda
        nan_col, inf_cols = (3 * 7) % k, [(3 * 6) % k, (3 * 6 + 22) % k]
        assert score.isnan().nonzero().flatten().tolist() == [nan_col] == want["score64"].isnan().nonzero().flatten().tolist()
        assert sorted(score.isinf().nonzero().flatten().tolist()) == sorted(inf_cols)
        fin = score.isfinite()
        assert ((score[fin].double() - want["score64"][fin]).abs() <= BOUND * want["score64"][fin]).all()
    # the NaN and the infinity stay in the state, and only where they are: a second batch's finite means do not replace them
    score, _ = run([x, torch.ones(3, k).bfloat16()], dev)
    assert score.isnan().nonzero().flatten().tolist() == [nan_col] and sorted(score.isinf().nonzero().flatten().tolist()) == sorted(inf_cols)
    assert (score[fin] >= 1.0).all()


def test_threshold_edges_fp16(dev):
    """the same sides in fp16, whose subnormals (below 2^-14) and largest value differ: thresholds between fp16 codes, a threshold in
    the subnormals, the largest finite row maximum"""
    k = 128
    rows = [(96.0, [7.0, 24.0, 6.96875, 23.875, 6.99609375, 7.00390625]), (3.0, [0.21875, 0.2177734375, 0.75, 0.74609375]),
            (3 * 2.0 ** -24, [2.0 ** -24, 2.0 ** -23]), (3 * 2.0 ** -14, [2.0 ** -16, 2.0 ** -15 + 2.0 ** -24, 2.0 ** -14]),
            (65504.0, [4776.0, 4780.0, 16376.0, 16368.0]), (0.0, []), (INF, [5.0, 65504.0, -INF]), (NAN, [1.0])]
    x = torch.zeros(len(rows) + 1, k)
    for r, (m, others) in enumerate(rows):
        for j, v in enumerate([m] + others):
            x[r, 3 * r + 11 * j] = v
    x[-1] = torch.randn(k, generator=torch.Generator().manual_seed(2))
    assert torch.equal(x[:-1].half().float().nan_to_num(1.5, 2.5, 3.5), x[:-1].nan_to_num(1.5, 2.5, 3.5))     # fp16 holds every planted value
    x = x.half()
    t4, t6 = co.thresholds(x.float().abs())
    assert (t4[0], t6[0], t4[1], t6[1]) == (7.0, 24.0, 0.21875, 0.75) and 0 < t6[2] < 2.0 ** -24 and t4[4] < 65504 < INF
    for lamda in (1.0, 0.7):
        for r in range(x.shape[0]):
            want = co.run([x[r:r + 1]], lamda)
            assert run([x[r:r + 1]], dev, lamda)[1] == [want["count4"], want["count6"]], (lamda, r)
        want = co.run([x], lamda)
        assert run([x], dev, lamda)[1] == [want["count4"], want["count6"]], lamda


# ---- 3. gauss ----------------------------------------------------------------------------------------------------------------------------
def gauss_batches():
    g = torch.Generator().manual_seed(0)
    x = torch.randn((512, 1024), generator=g)
    x[:, :13] *= 40
    x = x.bfloat16()
    return [x[:100], x[100:101], x[101:]]


def assert_order_agrees(got_score, want):
    """the stable argsort of the device's score against the oracle's fp64 scores: wherever two channels' fp64 scores differ by more than
    twice the bound they stand in the oracle's order; channels of exactly equal fp64 score take the same positions as a set"""
    s64 = want["score64"]
    got = torch.sort(got_score, stable=True).indices
    along = s64[got]
    before = torch.cummax(along, dim=0).values
    assert (before[:-1] - along[1:] <= 2 * BOUND * before[:-1]).all()
    for v in torch.unique(s64):
        tie = (s64 == v).nonzero().flatten()
        if len(tie) > 1 and float(torch.min((s64[s64 != v] - v).abs())) > 2 * BOUND * float(v):      # a tie that nothing else comes near
            pos = lambda order: sorted((order[:, None] == tie[None, :]).nonzero()[:, 0].tolist())
            assert pos(got) == pos(want["order"])


def test_gaussian_rows_with_outlier_channels(dev):
    batches = gauss_batches()
    want = co.run(batches)
    s64 = want["score64"]
    assert len(torch.unique(s64)) < s64.numel()                                        # exact ties: the one-row batch's means are bf16 values
    score, counts = run(batches, dev)
    assert counts == [want["count4"], want["count6"]]
    assert ((score.double() - s64).abs() <= BOUND * s64).all()
    assert_order_agrees(score, want)
    assert set(torch.sort(score, stable=True).indices[-13:].tolist()) == set(range(13))
    c = calib.Calibrator()
    for x in batches:
        c.observe("k", x.to(dev))
    order, p6, p8 = c.finish()
    assert (p6["k"], p8["k"]) == (want["p6"], want["p8"]) and torch.equal(order["k"], torch.sort(score, stable=True).indices)
    assert c.stats("k")[1:] == (want["count4"], want["count6"], want["numel"])


# ---- 4. bounds ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("rows, k, pad", [(R + 1, 128, 8), (5, 1152, 24), (2 * R + 3, 4096, 8)])
def test_nothing_outside_the_rows(dev, rows, k, pad, dtype):
    x = torch.randn(rows, k, generator=torch.Generator().manual_seed(rows)).to(dtype)
    big = torch.full((rows + 3, 8 + k + pad), NAN, dtype=dtype, device=dev)
    base = run([x], dev)
    for off, copied in ((8, False), (0, False), (3, True)):        # 16-byte aligned offsets with ld > K: read where they lie; off 3: copied
        big[:] = NAN
        view = big[:rows, off:off + k]
        view.copy_(x)
        assert (calib._rows(view)[0].data_ptr() == view.data_ptr()) == (not copied)
        got = run([view], dev)
        assert torch.equal(bits(got[0]), bits(base[0])) and got[1] == base[1], off
    assert not base[0].isnan().any()
    lead = torch.randn(2, 3, k, generator=torch.Generator().manual_seed(2)).to(dtype)          # [..., K] is seen as rows
    assert torch.equal(bits(run([lead], dev)[0]), bits(run([lead.reshape(6, k)], dev)[0]))


# ---- 5. state ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows, k", [(2 * R + 3, 1152), (257, 4096)])
def test_state_discipline(dev, rows, k):
    xs = [torch.randn(rows, k, generator=torch.Generator().manual_seed(s)).bfloat16().to(dev) for s in (3, 4)]
    first = run(xs, dev)
    poisoned = torch.full((calib.accumulate_workspace_bytes(rows, k),), 0xFF, dtype=torch.uint8, device=dev)
    again = run(xs, dev, workspace=poisoned)
    assert torch.equal(bits(first[0]), bits(again[0])) and first[1] == again[1]
    score, counts = fresh(k, dev, guard=8)
    score_all, counts_all = score._base, counts._base
    score_all[k:] = -3.0
    counts_all[2:] = -7
    for x in xs:
        calib.accumulate(x, score, counts)
    assert torch.equal(bits(score.cpu()), bits(first[0])) and counts.tolist() == first[1]
    assert (score_all[k:] == -3.0).all() and (counts_all[2:] == -7).all()
    kept = score_all.clone(), counts_all.clone()
    calib.accumulate(torch.empty(0, k, dtype=torch.bfloat16, device=dev), score, counts)      # no rows: the state is untouched
    calib.accumulate(torch.empty(4, 0, k, dtype=torch.float16, device=dev), score, counts)
    assert torch.equal(bits(score_all), bits(kept[0])) and torch.equal(counts_all, kept[1])
    with pytest.raises(RuntimeError, match="unsupported"):
        calib.accumulate(torch.zeros(4, 192, dtype=torch.bfloat16, device=dev), torch.zeros(192, device=dev), counts)
    with pytest.raises(RuntimeError, match="score must be"):
        calib.accumulate(xs[0], torch.zeros(k + 128, device=dev), counts)


# ---- 6. hooks ----------------------------------------------------------------------------------------------------------------------------
class ThreeLinears(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(256, 256)
        self.inner = torch.nn.ModuleDict({"b": torch.nn.Linear(256, 1152), "c": torch.nn.Linear(1152, 128)})

    def forward(self, x):
        return self.inner["c"](torch.tanh(self.inner["b"](torch.tanh(self.a(x)))))


def test_hooked_module_end_to_end(dev):
    torch.manual_seed(5)
    model = ThreeLinears().to(dev).to(torch.bfloat16)
    seen = {}
    plain = [m.register_forward_hook(lambda _m, args, _out, n=n: seen.setdefault(n + ".input", []).append(args[0].cpu()))
             for n, m in model.named_modules() if isinstance(m, torch.nn.Linear)]
    c = calib.Calibrator()
    handles = c.hook(model)
    assert len(handles) == 3
    with torch.no_grad():
        for tokens, g in ((5, 1), (64, 2), (130, 3)):
            model(torch.randn(1, tokens, 256, generator=torch.Generator().manual_seed(g)).bfloat16().to(dev))
    order, p6, p8 = c.finish()
    assert sorted(order) == sorted(p6) == sorted(p8) == ["a.input", "inner.b.input", "inner.c.input"] == sorted(seen)
    assert [order[k].numel() for k in sorted(order)] == [256, 256, 1152]
    for key, batches in seen.items():
        want = co.run(batches)
        score, c4, c6, numel = c.stats(key)
        assert (c4, c6, numel) == (want["count4"], want["count6"], want["numel"]) and numel == 199 * order[key].numel()
        assert ((score.cpu().double() - want["score64"]).abs() <= BOUND * want["score64"]).all()
        assert_order_agrees(score.cpu(), want)
        assert torch.equal(order[key], torch.sort(score.cpu(), stable=True).indices)
        assert (p6[key], p8[key]) == (want["p6"], want["p8"])
    c.remove()
    before = {k: (c.stats(k)[0].clone(),) + c.stats(k)[1:] for k in order}
    with torch.no_grad():
        model(torch.randn(1, 9, 256, generator=torch.Generator().manual_seed(4)).bfloat16().to(dev) * 50)
    for k, (score, c4, c6, numel) in before.items():
        assert torch.equal(bits(c.stats(k)[0]), bits(score)) and c.stats(k)[1:] == (c4, c6, numel)
    assert len(seen["a.input"]) == 4                                                   # the plain hooks were still on
    for h in plain:
        h.remove()
    prefixed = calib.Calibrator()
    prefixed.hook(model.inner, prefix="layers.0.")
    with torch.no_grad():
        model(torch.randn(3, 256, generator=torch.Generator().manual_seed(6)).bfloat16().to(dev))
    prefixed.remove()
    assert prefixed.keys() == ["layers.0.b.input", "layers.0.c.input"]
