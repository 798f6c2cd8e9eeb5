"""CPU tests of speculative sampling: the host side of mm_spec_sample_rows (include/micromix_spec.h: the symbols, the prototype, every
status without device work, the size function), the integer rule of csrc/mx_spec_rule.h run on the host against Python integers
(tools/spec_rule_host_check.cpp), the oracle's own invariants (tests/spec_oracle.py), the preconditions of the GPU cases of
tests/test_spec_sample_gpu.py, and chain_candidates on CPU tensors.  No kernel is launched here."""
import ctypes
import inspect
import os
import random
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from micromix_amd import _lib, mixedgemm
import sample_oracle as so
import spec_oracle as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD, UNS = _lib.MM_OK, _lib.MM_ERR_BAD_ARG, _lib.MM_ERR_UNSUPPORTED
C = _lib.MM_ARGMAX_CHUNK
ONE = sp.ONE


# ---- the C ABI and the Python ops ---------------------------------------------------------------------------------------------------------
def test_symbols_prototype_and_exports():
    """fails without the feature: the header, the symbols, SPEC_EXPORTS and the three Python names do not exist there"""
    lib = _lib.load()
    assert _lib.SPEC_EXPORTS == ("mm_spec_sample_rows_workspace_bytes", "mm_spec_sample_rows")
    others = set(_lib.EXPORTS) | set(_lib.DIAG_EXPORTS) | set(_lib.CALIB_EXPORTS) | set(_lib.LOGPROB_EXPORTS) | set(_lib.LOGITS_EXPORTS)
    assert not set(_lib.SPEC_EXPORTS) & others
    assert lib.mm_version() == 660 and sp.CHUNK == C
    v, i, ll, z = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_size_t
    assert hasattr(lib, "mm_spec_sample_rows") and hasattr(lib, "mm_spec_sample_rows_workspace_bytes")
    fn = lib.mm_spec_sample_rows
    assert fn.restype is i and list(fn.argtypes) == [v, ll, v, ll, i, i, v, v, v, v, v, v, v, v, v, v, z, v]
    size = lib.mm_spec_sample_rows_workspace_bytes
    assert size.restype is z and list(size.argtypes) == [i, i]
    assert _lib.constants(_lib.header_text("micromix_spec.h")) == {}                # no constant of the header reaches _lib
    for name in ("spec_sample_rows", "spec_sample_rows_workspace_bytes", "chain_candidates"):
        assert name in mixedgemm.__all__ and callable(getattr(mixedgemm, name)), name
    sig = inspect.signature(mixedgemm.spec_sample_rows).parameters
    assert list(sig) == ["logits", "draft_logits", "cand_tok", "u_accept", "u_resample", "temperature", "top_k", "top_p", "min_p", "out",
                         "accepted", "workspace"]
    assert all(sig[n].kind is inspect.Parameter.KEYWORD_ONLY and sig[n].default is None for n in list(sig)[5:])
    sig = inspect.signature(mixedgemm.chain_candidates).parameters
    assert list(sig) == ["draft_tok", "qo_indptr", "out"] and sig["out"].kind is inspect.Parameter.KEYWORD_ONLY
    import importlib.util
    spec = importlib.util.spec_from_file_location("dropin_mixedgemm_spec", os.path.join(ROOT, "micromix_amd", "dropin", "mixedgemm.py"))
    dropin = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dropin)
    assert dropin.spec_sample_rows is mixedgemm.spec_sample_rows and dropin.chain_candidates is mixedgemm.chain_candidates
    assert dropin.spec_sample_rows_workspace_bytes is mixedgemm.spec_sample_rows_workspace_bytes
    # chains only, and what to use for a tree: said in the header and in the docstring
    header = open(os.path.join(ROOT, "include", "micromix_spec.h")).read()
    for text in (header, mixedgemm.spec_sample_rows.__doc__):
        assert "tree" in text and "chains only" in text.lower() and "verify_greedy" in text


def test_statuses_without_device_work():
    """every row returns before a launch: the addresses are fakes or null"""
    lib = _lib.load()
    big = 1 << 40

    def spec(logits=16, ld=None, draft=32, draft_ld=None, rows=3, vocab=100, cand=16, ua=16, ur=16, T=16, k=16, p=16, q=16, out=16, acc=16,
             ws=64, ws_bytes=big):
        return lib.mm_spec_sample_rows(logits, vocab if ld is None else ld, draft, vocab if draft_ld is None else draft_ld, rows, vocab, cand,
                                       ua, ur, T, k, p, q, out, acc, ws, ws_bytes, None)

    assert spec(rows=0) == OK
    assert spec(rows=0, logits=None, draft=None, cand=None, ua=None, ur=None, out=None, acc=None, ws=None, ws_bytes=0) == OK
    for name in ("logits", "cand", "ua", "ur", "out"):
        assert spec(**{name: None}) == BAD, name
    assert spec(rows=-1) == BAD and spec(vocab=0) == BAD and spec(vocab=-5) == BAD
    assert spec(ld=99) == BAD and spec(draft_ld=99) == BAD and spec(ld=99, draft_ld=777) == BAD and spec(ld=777, draft_ld=99) == BAD
    for odd in (17, 19, 31):
        assert spec(logits=odd) == BAD and spec(draft=odd) == BAD, odd
    for name in ("cand", "ua", "ur", "T", "k", "p", "q", "out", "acc"):
        assert spec(**{name: 18}) == BAD, name                                     # 4-byte entries
    assert spec(vocab=(1 << 20) + 1) == UNS and spec(rows=_lib.MM_ARGMAX_MAX_ROWS + 1) == UNS
    assert spec(vocab=(1 << 20) + 1, ld=5) == BAD                                  # a refusal comes before a limit
    need = lib.mm_spec_sample_rows_workspace_bytes(3, 100)
    assert spec(ws=None) == BAD and spec(ws_bytes=need - 1) == BAD and spec(ws_bytes=0) == BAD and spec(ws=68, ws_bytes=need) == BAD
    # a draft_ld below vocab does not matter without draft logits
    assert spec(draft=None, draft_ld=0, ws_bytes=need - 1) == BAD and spec(draft=None, draft_ld=0, rows=0) == OK


def test_the_size_function():
    size = _lib.load().mm_spec_sample_rows_workspace_bytes
    need = size(3, 100)
    parts = lambda v: -(-v // C)
    assert need > 0 and need % 8 == 0 and need == size(3, C) and size(3, C + 1) > need
    assert size(0, 100) == 0 and size(-1, 100) == 0 and size(3, 0) == 0 and size(3, (1 << 20) + 1) == 0 and size(65536, 100) == 0
    # two matrices: twice mm_sample_rows' 3 KiB of histograms per part and 2 KiB per row, and change -- no scratch array of a row
    assert size(21, 128256) <= 21 * (parts(128256) * (2 * 3072 + 48) + 2 * 2080 + 64)
    assert size(21, 128256) >= 2 * _lib.load().mm_sample_rows_workspace_bytes(21, 128256)
    assert mixedgemm.spec_sample_rows_workspace_bytes(3, 100) == need


def test_python_argument_errors():
    lg = torch.zeros((3, 100), dtype=torch.bfloat16)
    u = torch.zeros((3,), dtype=torch.float32)
    cand = torch.zeros((3,), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mixedgemm.spec_sample_rows(lg, None, cand, u, u)
    with pytest.raises(TypeError, match="bfloat16"):
        mixedgemm.spec_sample_rows(lg.float(), None, cand, u, u)
    with pytest.raises(TypeError):
        mixedgemm.spec_sample_rows(None, None, cand, u, u)
    with pytest.raises(TypeError):
        mixedgemm.spec_sample_rows(lg, lg, cand, u, u, 0.7)                          # keyword-only


# ---- mx_spec_rule.h on the host against Python integers ------------------------------------------------------------------------------------
def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


@pytest.mark.skipif(shutil.which("c++") is None and shutil.which("g++") is None and shutil.which("clang++") is None, reason="needs a host C++ compiler")
def test_the_rule_header_on_the_host_equals_python_integers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    exe = str(tmp_path / "spec_rule_host_check")
    subprocess.run([cxx, "-std=c++20", "-O1", os.path.join(ROOT, "tools", "spec_rule_host_check.cpp"), "-o", exe], check=True)
    rng = random.Random(11)
    Us = [0, 1, 1 << 23, (1 << 24) - 1] + [rng.randrange(1 << 24) for _ in range(12)]
    queries, want = [], []
    # mulshift: 2^106-sized and 2^126-sized operands, small ones, low 24 bits all set or clear
    zs = [0, 1, (1 << 24) - 1, 1 << 24, (1 << 106) - 1, 1 << 105, (1 << 126) - 1, (1 << 126) - (1 << 24), ONE * ONE * 8]
    zs += [rng.randrange(1 << 106) for _ in range(40)] + [rng.randrange(1 << 126) for _ in range(40)]
    for z in zs:
        for U in Us:
            queries.append(f"m {z:x} {U:x}")
            want.append(f"{(U * z) >> 24:x}")
            assert sp.mulshift_split(z, U) == (U * z) >> 24
    # accept: random masses at their largest, and equality on the boundary -- U Qx Zp == 2^24 Px Zq exactly is a rejection, one less accepts
    for _ in range(200):
        Px, Qx = rng.randrange(ONE + 1), rng.randrange(ONE + 1)
        Zp, Zq = max(Px, ONE) + rng.randrange(1 << 62), max(Qx, ONE) + rng.randrange(1 << 62)
        U = rng.choice(Us)
        queries.append(f"a {Px:x} {Zp:x} {Qx:x} {Zq:x} {U:x}")
        want.append(str(int((U * Qx * Zp) >> 24 < Px * Zq)))
        assert sp.accept(Px, Zp, Qx, Zq, U) == (U * Qx * Zp < (Px * Zq) << 24)       # floor(a) < t  iff  a < t for an integer t
    for a, b in ((8, 4), (4, 8), (4, 4), (3, 5)):                                    # uniform on a and b tokens: p / q = b / a
        Px, Zp, Qx, Zq = ONE, a * ONE, ONE, b * ONE
        edge = -((-(1 << 24) * b) // a)                                              # the first U that is rejected: ceil(2^24 b / a)
        for U in (edge - 1, edge, edge + 1, 0, (1 << 24) - 1):
            if 0 <= U < 1 << 24:
                queries.append(f"a {Px:x} {Zp:x} {Qx:x} {Zq:x} {U:x}")
                want.append(str(int(U < edge)))
                assert sp.accept(Px, Zp, Qx, Zq, U) == (U < edge)
    for Px, Zp, Qx, Zq in ((0, ONE, ONE, ONE), (0, ONE, 0, ONE), (5, ONE, 0, ONE), (ONE, ONE, 1, 1), (ONE - 1, ONE, 1, 1), (ONE, 1 << 62, ONE, 1 << 62)):
        for U in Us[:4]:
            queries.append(f"a {Px:x} {Zp:x} {Qx:x} {Zq:x} {U:x}")
            want.append(str(int(sp.accept(Px, Zp, Qx, Zq, U))))
    for _ in range(100):
        Pi, Qi, Zp, Zq = rng.randrange(ONE + 1), rng.randrange(ONE + 1), ONE + rng.randrange(1 << 62), ONE + rng.randrange(1 << 62)
        queries.append(f"r {Pi:x} {Zp:x} {Qi:x} {Zq:x}")
        want.append(f"{max(0, Pi * Zq - Qi * Zp):x}")
    for u in (0.0, -1.0, float("nan"), 1.0, 7.0, 0.5, 0.5 - 2.0 ** -24, 0.5 - 2.0 ** -25, 2.0 ** -24, 2.0 ** -25, 1.0 - 2.0 ** -24, 0.3, float("inf")):
        queries.append(f"u {f32_bits(u):x}")
        want.append(f"{sp.U24(u):x}")
    run = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = run.stdout.split()
    assert len(got) == len(want)
    bad = [(q, g, w) for q, g, w in zip(queries, got, want) if g != w]
    assert not bad, bad[:5]
    assert sp.U24(0.5) == 1 << 23 and sp.U24(0.5 - 2.0 ** -24) == (1 << 23) - 1 and sp.U24(1.0) == (1 << 24) - 1 and sp.U24(float("nan")) == 0


# ---- the oracle's own invariants -------------------------------------------------------------------------------------------------------------
def test_a_rejected_row_has_residual_mass_and_never_returns_the_candidate():
    rng = random.Random(3)
    rejected = 0
    for trial in range(400):
        n = rng.randrange(2, 9)
        P = [rng.choice([0, rng.randrange(1, ONE + 1)]) for _ in range(n)]
        Q = [rng.choice([0, rng.randrange(1, ONE + 1)]) for _ in range(n)]
        P[rng.randrange(n)] = ONE
        Q[rng.randrange(n)] = ONE
        if trial % 4 == 0:
            Q = list(P)                                                             # the draft is the target
        x = rng.choice([i for i in range(n) if Q[i] > 0] if trial % 3 else range(n))
        Ua = rng.choice([0, 1, 1 << 23, (1 << 24) - 1, rng.randrange(1 << 24)])
        Zp, Zq = sum(P), sum(Q)
        if sp.accept(P[x], Zp, Q[x], Zq, Ua):
            assert P[x] > 0
            continue
        rejected += 1
        R = sp.residual(P, Zp, Q, Zq)
        assert R[x] == 0
        if Q[x] > 0:
            assert sum(R) > 0 and sum(R) == sum(max(0, q * Zp - p * Zq) for p, q in zip(P, Q))
        else:
            assert P[x] == 0
        assert sum(R) < 1 << 126
        for ur in (0.0, 0.999999, rng.random()):
            tok, acc = sp.spec_sample(P, Q, x, Ua / 2.0 ** 24, ur, fallback=P.index(ONE))
            assert acc == 0 and tok != x and P[tok] > 0
    assert rejected > 100
    # the header's consequences: Q_x = 0 < P_x always accepts, P_x = 0 always rejects, the draft equal to the target always accepts
    assert all(sp.accept(1, 5 * ONE, 0, ONE, U) and not sp.accept(0, ONE, 1, 5 * ONE, U) for U in (0, (1 << 24) - 1))
    assert all(sp.accept(p, 7 * ONE + 3, p, 7 * ONE + 3, (1 << 24) - 1) for p in (1, 12345, ONE))
    # one-hot: a target that is one-hot at x always accepts; otherwise the residual is P with x removed
    assert sp.spec_sample([0, ONE, 0], None, 1, 1.0, 0.3) == (1, 1)
    assert sp.residual([ONE, 5, 7], ONE + 12, [0, 1, 0], 1) == [ONE, 0, 7]


def acceptance_is_rounded_up(a, b):
    """the number of U that accept a shared token of uniform rows of a and b tokens is ceil(2^24 min(1, b / a))"""
    edge = min(1 << 24, -((-(1 << 24) * b) // a))
    lo, hi = 0, 1 << 24                                                             # accept is monotone in U: bisect the first rejection
    while lo < hi:
        mid = (lo + hi) // 2
        if sp.accept(ONE, a * ONE, ONE, b * ONE, mid):
            lo = mid + 1
        else:
            hi = mid
    return lo == edge


def test_the_acceptance_probability_is_min_1_p_over_q_rounded_up_to_the_grid():
    assert all(acceptance_is_rounded_up(a, b) for a, b in ((8, 4), (4, 8), (3, 7), (7, 3), (5, 5), (1000, 3)))


@pytest.mark.parametrize("vocab", [C - 1, C, C + 1, 2 * C + 5])
@pytest.mark.parametrize("a, b", [(8, 4), (4, 8), (4, 4), (8, 8)])
def test_the_exact_family_by_integer_arithmetic_alone(vocab, a, b):
    """the facts the GPU test of the same family relies on, from the oracle: the boundary pair, what is always accepted and always
    rejected, the residual weights, and the distribution test -- every x of B against the grid of (u_accept, u_resample), weighted by
    q(x) = 1 / |B|, returns every token of A equally often: the output is distributed as p, exactly"""
    A, B = sp.exact_sets(vocab, a, b)
    assert len(A) == a and len(B) == b and len(set(A) & set(B)) == 2 and max(A + B) < vocab
    for e in range(C, vocab, C):
        assert {e - 1, e} <= set(A) | set(B)
    tb, db = sp.uniform_row(vocab, A), sp.uniform_row(vocab, B)
    P, Q = sp.masses(tb), sp.masses(db)
    assert sum(P) == a * ONE and sum(Q) == b * ONE
    shared, only_a, only_b = sorted(set(A) & set(B)), sorted(set(A) - set(B)), sorted(set(B) - set(A))
    R = sp.residual(P, sum(P), Q, sum(Q))
    unit = ONE * ONE
    assert all(R[i] == max(b - a, 0) * unit for i in shared) and all(R[i] == b * unit for i in only_a)
    assert sum(R) == (2 * max(b - a, 0) + (a - 2) * b) * unit
    for x in shared:
        if (a, b) == (8, 4):
            assert sp.spec_row(tb, db, x, 0.5 - 2.0 ** -24, 0.3)[1] == 1 and sp.spec_row(tb, db, x, 0.5, 0.3)[1] == 0
        else:
            assert all(sp.spec_row(tb, db, x, u, 0.3) == (x, 1) for u in (0.0, 0.5, 1.0 - 2.0 ** -24, 1.0))
    for x in only_b:
        assert all(sp.spec_row(tb, db, x, u, 0.3)[1] == 0 for u in (0.0, 0.5, 1.0))
    n, n2 = DIST_GRID
    counts = np.zeros(vocab, dtype=np.int64)
    for x in B:
        for j in range(n):
            for k in range(n2):
                tok, acc = sp.spec_row(tb, db, x, np.float32((j + 0.5) / n), np.float32((k + 0.5) / n2))
                counts[tok] += 1
    assert counts.sum() == b * n * n2 and (b * n * n2) % a == 0
    assert sorted(np.flatnonzero(counts).tolist()) == A and set(counts[A].tolist()) == {b * n * n2 // a}
    # the expected acceptance of the pair, as arithmetic: sum min(p, q) against exact matching's sum p q
    got = sp.expected_acceptance([1 / a] * 2 + [1 / a] * (a - 2) + [0] * (b - 2), [1 / b] * 2 + [0] * (a - 2) + [1 / b] * (b - 2))
    assert got == pytest.approx((2 * min(1 / a, 1 / b), 2 / (a * b)))


DIST_GRID = (2, 6)       # u_accept = (j + 0.5) / 2 splits at 1/2; u_resample = (k + 0.5) / 6 splits the 24 residual units at sixths


def test_the_one_hot_form_on_the_exact_family():
    vocab = C + 1
    A, _ = sp.exact_sets(vocab, 4, 4)
    tb = sp.uniform_row(vocab, A)
    x = A[1]
    # accept iff mulshift(Zp, U) < P_x: u < 1/4 for four equal tokens
    assert sp.spec_row(tb, None, x, 0.25 - 2.0 ** -24, 0.0) == (x, 1) and sp.spec_row(tb, None, x, 0.25, 0.0) == (A[0], 0)
    rest = [c for c in A if c != x]
    assert [sp.spec_row(tb, None, x, 0.9, (k + 0.5) / 3)[0] for k in range(3)] == rest
    outside = next(c for c in range(vocab) if c not in A)
    assert sp.spec_row(tb, None, outside, 0.0, 0.5)[1] == 0
    # a draft row in the greedy case is the one-hot form
    nan_row = np.full(vocab, 0x7FC0, dtype=np.uint16)
    assert sp.spec_row(tb, nan_row, x, 0.1, 0.0) == sp.spec_row(tb, None, x, 0.1, 0.0) == (x, 1)
    assert sp.spec_row(tb, nan_row, x, 0.6, 0.7) == sp.spec_row(tb, None, x, 0.6, 0.7)
    # a greedy target: argmax, and 1 / 0 / -1 as it equals the candidate
    assert sp.spec_row(tb, None, A[0], 0.9, 0.9, T=0.0) == (A[0], 1) and sp.spec_row(tb, None, A[1], 0.0, 0.9, T=0.0) == (A[0], 0)
    assert sp.spec_row(tb, None, -1, 0.0, 0.9, T=0.0) == (A[0], -1)
    # no candidate: mm_sample_rows' draw
    assert [sp.spec_row(tb, None, c, 0.0, 0.6)[0] for c in (-1, vocab, None)] == [so.sample(tb, 0.6)] * 3 == [A[2]] * 3


# ---- the Gaussian cases of the GPU file ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filters", [False, True])
def test_the_gaussian_seed_leaves_at_most_one_row_in_sixteen_undecided(filters):
    """the committed seed and noise scale, from the oracle alone: at most 1 / 16 of the rows have more than one admissible decision,
    at most 1 / 16 more than one admissible token; both decisions occur, and neither side is greedy"""
    bits, draft, cand, par = sp.gaussian_case(filters)
    sets = sp.gaussian_admissible(filters)
    rows = sp.GAUSSIAN_ROWS
    assert bits.shape == draft.shape == (rows, sp.GAUSSIAN_VOCAB) and rows <= 16
    assert not any(so.is_greedy(bits[i], par["T"][i]) or so.is_greedy(draft[i], par["T"][i]) for i in range(rows))
    assert all(d and t for d, t, _ in sets)
    assert sum(len(d) > 1 for d, _, _ in sets) * 16 <= rows, [d for d, _, _ in sets]
    assert sum(len(t) > 1 for _, t, _ in sets) * 16 <= rows, [sorted(t)[:4] for _, t, _ in sets]
    decided = [next(iter(d)) for d, _, _ in sets if len(d) == 1]
    assert decided.count(1) >= 3 and decided.count(0) >= 3, decided
    for i, (d, t, kept) in enumerate(sets):
        assert all(kept[tok] for tok in t), i                                     # every admissible output lies in the target's kept set
        if d == {0}:
            assert int(cand[i]) not in t
    assert len({float(par["T"][i]) for i in range(rows)}) == rows


# ---- chain_candidates ------------------------------------------------------------------------------------------------------------------------
def test_chain_candidates_on_cpu_tensors():
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)
    for qo in ([0, 4, 4, 8, 12], [0, 0, 3, 3, 3, 5], [0, 1, 2, 3], [0, 0], [0, 5], [0, 0, 0, 2, 2]):
        T = qo[-1]
        draft = [100 + 3 * t for t in range(T)]
        want = sp.chain_candidates(draft, qo)
        got = mixedgemm.chain_candidates(i32(draft), i32(qo))
        assert got.dtype is torch.int32 and got.tolist() == want, qo
        out = torch.full((T,), 77, dtype=torch.int32)
        assert mixedgemm.chain_candidates(i32(draft), i32(qo), out=out) is out and out.tolist() == want
    assert sp.chain_candidates([5, 6, 7, 8, 9], [0, 0, 3, 3, 5]) == [6, 7, -1, 9, -1]
    with pytest.raises(TypeError, match="int32"):
        mixedgemm.chain_candidates(torch.zeros(3, dtype=torch.int64), i32([0, 3]))
    with pytest.raises(RuntimeError, match="out must be"):
        mixedgemm.chain_candidates(i32([1, 2, 3]), i32([0, 3]), out=torch.zeros(2, dtype=torch.int32))


def test_the_chain_walk_is_the_speculative_algorithm():
    """on a toy table of row results: the accepted prefix, the redraw at the first rejection, the plain sample after the leaf, a root
    that does not match, an empty sequence and a prompt chunk"""
    draft = [10, 11, 12, 13, 20, 21, 22, 23, 30, 31, 32, 33]
    qo = [0, 4, 4, 8, 12]
    table = {(0, 11): (11, 1), (1, 12): (12, 1), (2, 13): (99, 0), (4, 21): (21, 1), (5, 22): (22, 1), (6, 23): (23, 1), (7, None): (55, -1),
             (11, None): (66, -1)}
    walk = sp.chain_walk(lambda t, x: table[(t, x)], draft, [10, 7, 20, -1], qo)
    assert walk == [(3, 99), (0, 7), (4, 55), (4, 66)]
    assert sp.chain_walk(lambda t, x: table[(t, x)], draft, [11, 7, 20, -1], qo)[0] == (0, 11)
