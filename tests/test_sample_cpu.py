"""CPU tests of the sampler: the host side of mm_sample_rows (symbols, every status without device work, Python argument errors), the
numpy oracle itself (tests/sample_oracle.py: its kept set against an HF-style sort / cumsum implementation in torch, its greedy cases
against torch.argmax) and, in fp64, the preconditions of the GPU cases of tests/test_sample_gpu.py.  No kernel is launched here."""
import inspect
import math

import numpy as np
import pytest
import torch

from micromix_amd import _lib, mixedgemm
from micromix_amd.kvcache import PagedKVCache
import sample_cases as sc
import sample_oracle as so

OK, BAD, UNS = _lib.MM_OK, _lib.MM_ERR_BAD_ARG, _lib.MM_ERR_UNSUPPORTED
C = _lib.MM_ARGMAX_CHUNK


# ---- the C ABI and the Python op ---------------------------------------------------------------------------------------------------------
def test_symbols_declared_and_exported_and_the_version_stays():
    lib = _lib.load()
    header = open(inspect.getsourcefile(_lib).replace("micromix_amd/_lib.py", "include/micromix_hip.h")).read()
    for name in ("mm_sample_rows_workspace_bytes", "mm_sample_rows"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and f" {name}(" in header, name
    assert lib.mm_version() == 660 and sc.CHUNK == C
    for name in ("sample_rows", "sample_rows_workspace_bytes"):
        assert name in mixedgemm.__all__ and callable(getattr(mixedgemm, name))
    sig = inspect.signature(mixedgemm.sample_rows).parameters
    assert list(sig) == ["logits", "u", "temperature", "top_k", "top_p", "min_p", "out", "workspace"]
    assert all(sig[n].kind is inspect.Parameter.KEYWORD_ONLY and sig[n].default is None for n in list(sig)[2:])
    import importlib.util
    spec = importlib.util.spec_from_file_location("dropin_mixedgemm", inspect.getsourcefile(_lib).replace("_lib.py", "dropin/mixedgemm.py"))
    dropin = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dropin)
    assert dropin.sample_rows is mixedgemm.sample_rows and dropin.sample_rows_workspace_bytes is mixedgemm.sample_rows_workspace_bytes
    assert "sample_rows" in PagedKVCache.verify_launch.__doc__


def test_statuses_without_device_work():
    """every row returns before a launch: the addresses are fakes or null"""
    lib = _lib.load()
    big = 1 << 40

    def smp(logits=16, rows=3, vocab=100, ld=None, u=16, T=16, k=16, p=16, q=16, out=16, ws=64, ws_bytes=big):
        return lib.mm_sample_rows(logits, rows, vocab, vocab if ld is None else ld, u, T, k, p, q, out, ws, ws_bytes, None)

    assert smp(rows=0) == OK and smp(rows=0, logits=None, u=None, out=None, ws=None, ws_bytes=0) == OK
    assert smp(logits=None) == BAD and smp(u=None) == BAD and smp(out=None) == BAD
    assert smp(rows=-1) == BAD and smp(vocab=0) == BAD and smp(vocab=-5) == BAD and smp(ld=99) == BAD
    for odd in (17, 19, 31):
        assert smp(logits=odd) == BAD, odd
    for name in ("u", "T", "k", "p", "q", "out"):
        assert smp(**{name: 18}) == BAD, name                                      # 4-byte entries
    assert smp(vocab=(1 << 20) + 1) == UNS and smp(rows=_lib.MM_ARGMAX_MAX_ROWS + 1) == UNS
    need = lib.mm_sample_rows_workspace_bytes(3, 100)
    parts = lambda v: -(-v // C)
    assert need > 0 and need % 8 == 0 and need == lib.mm_sample_rows_workspace_bytes(3, C)
    assert lib.mm_sample_rows_workspace_bytes(3, C + 1) > need                     # a second part
    # 3 KiB of histograms per part, 2 KiB per row, and change: no 128 k-entry scratch array of a row
    assert lib.mm_sample_rows_workspace_bytes(21, 128256) <= 21 * (parts(128256) * (3072 + 16) + 2048 + 64)
    assert lib.mm_sample_rows_workspace_bytes(0, 100) == 0 and lib.mm_sample_rows_workspace_bytes(3, 0) == 0
    assert lib.mm_sample_rows_workspace_bytes(3, (1 << 20) + 1) == 0
    assert smp(ws=None) == BAD and smp(ws_bytes=need - 1) == BAD and smp(ws_bytes=0) == BAD and smp(ws=68, ws_bytes=need) == BAD
    assert smp(ws=None, ws_bytes=need) == BAD


def test_python_argument_errors():
    lg = torch.zeros((3, 100), dtype=torch.bfloat16)
    u = torch.zeros((3,), dtype=torch.float32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mixedgemm.sample_rows(lg, u)
    with pytest.raises(TypeError, match="bfloat16"):
        mixedgemm.sample_rows(lg.float(), u)
    with pytest.raises(TypeError):
        mixedgemm.sample_rows(None, u)
    assert mixedgemm.sample_rows_workspace_bytes(3, 100) == _lib.load().mm_sample_rows_workspace_bytes(3, 100)


# ---- the oracle against an HF-style implementation -----------------------------------------------------------------------------------------
def hf_keep(bits, T, k, p, q):
    """temperature, TopKLogitsWarper, TopPLogitsWarper and MinPLogitsWarper as transformers applies them, in float64 torch: a sort and
    a cumulative sum.  top-p sees the distribution renormalised over what top-k left; min-p is relative to the largest probability, so
    its place in the chain does not matter and it is applied to the scaled logits directly"""
    x = torch.from_numpy(so.values(bits)) / T
    keep = torch.ones_like(x, dtype=torch.bool)
    if k is not None and 1 <= k < len(x):
        keep &= x >= torch.topk(x, k).values[-1]
    if p is not None and p < 1:
        s, order = torch.sort(x.masked_fill(~keep, -math.inf), descending=False)
        cum = torch.softmax(s, dim=0).cumsum(0)
        remove = cum <= 1.0 - max(p, 0.0)
        remove[-1] = False                                   # min_tokens_to_keep = 1
        keep &= ~torch.zeros_like(remove).scatter(0, order, remove)
    if q is not None and 0 < q <= 1:
        keep &= torch.softmax(x, dim=0) >= q * torch.softmax(x, dim=0).max()
    return keep.numpy()


def random_params(rng):
    return (float(rng.choice([0.5, 0.8, 1.0, 1.7])), int(rng.choice([0, 1, 5, 40, 150])) or None,
            float(rng.choice([1.0, 0.3, 0.7, 0.9, 0.97])), float(rng.choice([0.0, 0.001, 0.02, 0.2])) or None)


def test_kept_set_equals_hf_on_rows_without_a_tie_at_a_threshold():
    rng = np.random.default_rng(5)
    compared = 0
    for _ in range(60):
        bits = so.bf16_bits(rng.standard_normal(200) * 3.0)
        bits = bits[np.unique(so.values(bits), return_index=True)[1]]                # no ties at all
        T, k, p, q = random_params(rng)
        cls, w, t, end_k, end_p, end_q, mass = so.prefix_ends(bits, T, k, p, q)
        if p < 1 and min(abs(m - p * mass[end_k]) for m in mass) < 1e-9 * mass[-1]:
            continue                                         # a prefix that ends on the target in fp64: either answer is rounding
        got, want = so.kept_mask(bits, T, k, p, q), hf_keep(bits, T, k, p, q)
        assert np.array_equal(got, want), (T, k, p, q, np.flatnonzero(got != want))
        compared += 1
    assert compared >= 50


def test_kept_set_differs_from_hf_only_inside_one_class_on_rows_with_ties():
    rng = np.random.default_rng(6)
    differed = 0
    for _ in range(60):
        bits = so.bf16_bits(np.round(rng.standard_normal(200) * 3.0))                 # integers: ties everywhere
        T, k, p, q = random_params(rng)
        got, want = so.kept_mask(bits, T, k, p, q), hf_keep(bits, T, k, p, q)
        assert not (want & ~got).any(), "a superset of HF's set"
        extra = np.flatnonzero(got & ~want)
        assert len(set(so.values(bits)[extra].tolist())) <= 1, "by at most the rest of one tie class"
        differed += bool(len(extra))
        if p >= 1:
            assert not len(extra), "top-k and min-p are HF's exactly"
    assert differed >= 3


def test_greedy_cases_equal_torch_argmax():
    rng = np.random.default_rng(7)
    bits = so.bf16_bits(np.round(rng.standard_normal((8, 97)) * 2.0))
    bits[1, 40] = 0x7FC0                                     # NaN
    bits[2, 41] = 0x7F80                                     # +inf
    bits[3, :] = 0xFF80                                      # only -inf
    bits[4, 13] = 0xFFC0                                     # -NaN
    to_torch = lambda b: torch.from_numpy(b.view(np.int16).copy()).view(torch.bfloat16)
    want = torch.argmax(to_torch(bits), dim=1).numpy()
    for r in range(8):
        for T in ((1.0,) if 1 <= r <= 4 else (0.0, -1.0, float("nan"))):
            assert so.is_greedy(bits[r], T) and so.sample(bits[r], 0.9, T, 5, 0.5, 0.1) == want[r], (r, T)
            assert so.admissible(bits[r], 0.9, T) == {int(want[r])}
    assert not so.is_greedy(bits[0], 1.0) and not so.is_greedy(bits[0], float("inf"))


def test_the_rule_on_hand_written_rows():
    bits = so.bf16_bits(np.array([1.0, 3.0, 3.0, 2.0, -1.0], dtype=np.float32))
    bits = np.concatenate([bits, np.array([0xFF80], dtype=np.uint16)])
    assert so.kept_mask(bits, 1.0, 1, None, None).tolist() == [False, True, True, False, False, False]      # the tie is kept whole
    assert so.kept_mask(bits, 1.0, 3, None, None).tolist() == [False, True, True, True, False, False]
    assert so.kept_mask(bits, 1.0, None, 0.0, None).tolist() == [False, True, True, False, False, False]
    assert so.kept_mask(bits, 1.0, None, None, 0.3).tolist() == [False, True, True, True, False, False]     # e^-1 = 0.37, e^-2 = 0.14
    assert so.kept_mask(bits, 1.0, 6, None, None).all() and so.kept_mask(bits, 1.0, 0, 1.0, 0.0).all()
    Z = 2 + math.exp(-1) + math.exp(-2) + math.exp(-4)
    assert so.sample(bits, 0.0) == 0 and so.sample(bits, (math.exp(-2) + 0.5) / Z) == 1 and so.sample(bits, float("nan")) == 0
    assert so.sample(bits, 1.0) == 4 and so.sample(bits, 7.0) == 4                                     # clamped; -inf is never drawn
    assert so.clamp_u(1.0) == 1.0 - 2.0 ** -24 and so.clamp_u(-3.0) == 0.0
    assert so.admissible(bits, 0.3) == {so.sample(bits, 0.3)}
    # a threshold inside the bound: two prefixes are admissible, and so is a token of each
    two = so.bf16_bits(np.array([0.0, 0.0], dtype=np.float32))
    assert so.admissible_ends(two, 1.0)[0] == [1] and so.admissible(two, 0.5) == {0, 1} and so.admissible(two, 0.4999) == {0}


# ---- preconditions of the GPU cases, in fp64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(len(sc.TRIPLES)))
def test_every_filter_case_decides_with_a_margin(which):
    """every comparison of a filter case is at least MARGIN = 1e-3 away from its threshold, relative to the threshold: top-p's prefix
    masses from p * Z_k, min-p's weights from q; and the draw: u * Z lies in the last kept token's interval at least MARGIN of that
    token's weight above its lower end (its upper end is the end of the row, below which u < 1 keeps every device).  The expected
    token is the rule's, and it is the last token of the class the case names"""
    bits, T, rows, last = sc.filter_case(which)
    values = sc.TRIPLES[which][1]
    for label, k, p, q, kept in rows:
        cls, w, t, end_k, end_p, end_q, mass = so.prefix_ends(bits, T, k, p, q)
        assert [c[0] for c in cls[:3]] == [float(v) for v in values] and [len(c[1]) for c in cls[:3]] == [3, 5, 1000], label
        end = min(end_k, end_p, end_q)
        assert min(end, 3) == kept, (label, end_k, end_p, end_q)
        fk, fp, fq = so.filters(k, p, q, len(bits))
        if fp is not None and fp > 0:
            tgt = fp * mass[end_k]
            assert all(abs(m - tgt) >= sc.MARGIN * tgt for m in mass[:end_k + 1]), label
        if fq is not None:
            # (the maximum's weight is exactly 1 on the device as well, and q <= 1 keeps it)
            assert all(abs(w[c[1][0]] - fq) >= sc.MARGIN * fq for c in cls[1:] if w[c[1][0]] > 0), label
        want = so.sample(bits, sc.U_LAST, T, k, p, q)
        assert want == last[kept - 1], label
        keep = so.kept_mask(bits, T, k, p, q)
        Z = float(w[keep].sum())
        assert float(sc.U_LAST) * Z - (Z - w[want]) >= sc.MARGIN * w[want], label
        assert so.admissible(bits, sc.U_LAST, T, k, p, q) == {want}, label
    # a kernel that ignores a filter lands elsewhere
    assert len({last[r[4] - 1] for r in rows}) == 3


def test_the_bound_is_what_the_docstring_derives():
    assert so.rel_error(np.array([0.0]))[0] == pytest.approx(2.0 ** -23, rel=2e-3)
    assert so.rel_error(np.array([-44.0]))[0] == pytest.approx(44 * math.log(2) * 2.0 ** -22 + 2.0 ** -23, rel=2e-3)
    assert so.rel_error(np.array([-44.0]))[0] < 7.5e-6
    bits, par = so.gaussian_case(32000, 4, 1)
    assert 2e-7 < so.eps_of(bits[0], 1.0) < 6e-6


@pytest.mark.parametrize("vocab", [32000, 2 * C + 5])
def test_most_gaussian_rows_have_one_admissible_token(vocab):
    sets = so.gaussian_admissible(vocab)
    single = sum(len(s) == 1 for s in sets)
    assert all(len(s) >= 1 for s in sets) and single >= 0.9 * len(sets), f"{single} of {len(sets)} rows with one admissible token"
    bits, par = so.gaussian_case(vocab, so.GAUSSIAN_ROWS, vocab)
    for name in ("u", "T", "k", "p", "q"):
        on = [x for r, x in enumerate(par[name].tolist()) if name in "uT" or r % 8 not in {"k": (0, 3), "p": (1,), "q": (2,)}[name]]
        assert len(set(on)) == len(on) >= so.GAUSSIAN_ROWS - 16, name                # parameters that all differ within the call
    for r in (0, 1, 2, 3, 4):                                                        # the rule's own token is admissible
        assert so.sample(bits[r], par["u"][r], par["T"][r], par["k"][r], par["p"][r], par["q"][r]) in sets[r]


def test_the_stratified_and_long_rows_have_mostly_one_admissible_token():
    sets = so.stratified_admissible()
    assert sum(len(s) == 1 for s in sets) >= 0.9 * len(sets)
    assert len(set.union(*sets)) >= 20, "the draws must spread over the kept set"
    for vocab in (128256, 152064):
        bits, par = so.long_row(vocab)
        assert len(so.admissible(bits, par["u"], par["T"], par["k"], par["p"], par["q"])) == 1
