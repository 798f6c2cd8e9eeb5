"""CPU tests of the seeded uniform numbers (include/micromix_random.h: mm_uniform_rows): the oracle against Random123's known-answer
vectors; the vectors that pin which word goes where; the header, the symbol, the prototype and the Python names; every status of the
call without device work; mixedgemm.uniform_rows on CPU tensors -- the rule in plain Python -- against tests/random_oracle.py.
Every assertion is equality.  No kernel is launched here."""
import ctypes
import inspect
import os
import random

import pytest
import torch

from micromix_amd import _lib, mixedgemm
import random_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD, UNS = _lib.MM_OK, _lib.MM_ERR_BAD_ARG, _lib.MM_ERR_UNSUPPORTED
i32 = lambda x: torch.tensor(x, dtype=torch.int32)
i64 = lambda x: torch.tensor(x, dtype=torch.int64)
words = lambda text: [int(w, 16) for w in text.split()]

# (seed, pos, sub, domain, n, the words, u * 2^24 or None): computed with a from-scratch Python Philox when the feature was specified
INTERFACE_VECTORS = [
    (0x0123456789ABCDEF, 1000, 0, 7, 8, words("32b728dd 3d15629c 8475daa8 6cf7fda5 9bbec9b1 4e83e918 86baab0d f1a00fd4"),
     [3323688, 4003170, 8680922, 7141373, 10206921, 5145577, 8829611, 15835151]),
    (-1, -1, -1, 0xFFFFFFFF, 4, words("1feaf384 39714dd8 b671a4cc 36fbd643"), None),
]


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------------
def test_the_oracle_gives_the_known_answers_of_random123():
    f = 0xFFFFFFFF
    assert list(ro.philox4x32_10((0, 0, 0, 0), (0, 0))) == words("6627e8d5 e169c58d bc57ac4c 9b00dbd8")
    assert list(ro.philox4x32_10((f, f, f, f), (f, f))) == words("408f276d 41c83b0e a20bc7c6 6d5451fd")
    assert list(ro.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == words(
        "d16cfe09 94fdcceb 5001e420 24126ea1")


def test_the_oracle_puts_every_word_in_its_place():
    for seed, pos, sub, domain, n, bits, u24 in INTERFACE_VECTORS:
        got_u, got_bits = ro.uniform_rows([seed], [pos], n, [sub], None, domain)
        assert [s[0] for s in got_bits] == bits and [s[0] for s in got_u] == [w >> 8 for w in bits]
        assert u24 is None or [s[0] for s in got_u] == u24
    # the blocks are counter word 2, the domain word 3, the key the seed's halves, low first
    assert ro.words(0x0000000200000001, 3, 4, 5, 8) == list(ro.philox4x32_10((3, 4, 0, 5), (1, 2))) + list(ro.philox4x32_10((3, 4, 1, 5), (1, 2)))


# ---- the C ABI and the Python names ---------------------------------------------------------------------------------------------------
def test_symbol_prototype_and_exports():
    """fails without the feature: the header, the symbol, RANDOM_EXPORTS and the Python name do not exist there"""
    lib = _lib.load()
    assert _lib.RANDOM_EXPORTS == ("mm_uniform_rows",)
    others = (set(_lib.EXPORTS) | set(_lib.DIAG_EXPORTS) | set(_lib.CALIB_EXPORTS) | set(_lib.LOGPROB_EXPORTS) | set(_lib.LOGITS_EXPORTS)
              | set(_lib.SPEC_EXPORTS) | set(_lib.KVSTEP_EXPORTS) | set(_lib.TOKENS_EXPORTS))
    assert not set(_lib.RANDOM_EXPORTS) & others
    assert lib.mm_version() == 660
    v, i, u, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_longlong
    assert hasattr(lib, "mm_uniform_rows")
    assert lib.mm_uniform_rows.restype is i and list(lib.mm_uniform_rows.argtypes) == [v, v, i, v, v, i, i, u, v, v, ll, v]
    consts = _lib.constants(_lib.header_text("micromix_random.h"))
    assert consts == _lib.RANDOM == dict(MM_UNIFORM_MAX_N=ro.MAX_N, MM_UNIFORM_MAX_ROWS=ro.MAX_ROWS) and ro.MAX_ROWS == 1 << 24
    assert not any(hasattr(_lib, n) for n in consts)
    assert "uniform_rows" in mixedgemm.__all__ and callable(mixedgemm.uniform_rows)
    sig = inspect.signature(mixedgemm.uniform_rows).parameters
    assert list(sig) == ["seed", "pos", "n", "sub", "row_seq", "domain", "out", "bits"]
    assert all(sig[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig)[2:])
    assert (sig["n"].default, sig["sub"].default, sig["row_seq"].default, sig["domain"].default, sig["out"].default, sig["bits"].default) == (
        3, None, None, 0, None, False)
    import importlib.util
    spec = importlib.util.spec_from_file_location("dropin_mixedgemm_random", os.path.join(ROOT, "micromix_amd", "dropin", "mixedgemm.py"))
    dropin = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dropin)
    assert dropin.uniform_rows is mixedgemm.uniform_rows
    header = open(os.path.join(ROOT, "include", "micromix_random.h")).read()
    assert "THE INDEX IN THE HISTORY AT WHICH THE TOKEN THAT ROW DECIDES WILL BE COMMITTED" in header
    assert "NO STATE, NO ATOMIC, NO WORKSPACE" in header and "THE STREAMS ARE ROWS OF out" in header
    assert "EVERY u LIES ON THE 2^-24 GRID" in header and "Sibling nodes of a tree share a position" in header


def test_the_source_is_a_product_source():
    from micromix_amd import build
    assert "random.hip" in build.SOURCES and any(h.endswith("micromix_random.h") for h in build.HEADERS)
    text = open(os.path.join(build.CSRC, "random.hip")).read()
    assert "__umulhi" in text and "asm" not in text and "atomic" not in text.replace("no atomic", "") and "__shared__" not in text


def test_statuses_without_device_work():
    """every row returns before a launch: the addresses are fakes or null"""
    lib = _lib.load()

    def call(seed=64, sub=16, batch=3, seq=32, pos=48, rows=5, n=3, domain=0, out=80, bits=96, ld=5):
        return lib.mm_uniform_rows(seed, sub, batch, seq, pos, rows, n, domain, out, bits, ld, None)

    assert call(rows=0, ld=0) == OK and call(rows=0) == OK
    assert call(rows=0, ld=0, seed=None, sub=None, seq=None, pos=None, out=None, bits=None, batch=0) == OK
    assert call(rows=-1) == BAD and call(batch=-1) == BAD and call(n=0) == BAD and call(n=-3) == BAD
    assert call(ld=4) == BAD and call(ld=-1) == BAD and call(rows=0, ld=-1) == BAD
    assert call(out=None, bits=None) == BAD and call(seed=None) == BAD and call(pos=None) == BAD
    assert call(rows=0, n=0) == BAD and call(rows=0, batch=-1) == BAD                          # refused whatever rows is
    for off in range(1, 8):
        assert call(seed=64 + off) == BAD, off                                                  # 8-byte entries
    for name in ("sub", "seq", "pos", "out", "bits"):
        for off in (1, 2, 3):
            assert call(**{name: 192 + off}) == BAD, name                                      # 4-byte entries
    assert call(n=17) == UNS and call(rows=(1 << 24) + 1, ld=1 << 25) == UNS and call(n=1 << 30) == UNS
    assert call(n=17, rows=0) == UNS                                                            # a limit comes before "nothing to do"
    assert call(n=17, pos=None) == BAD and call(rows=(1 << 24) + 1, ld=5) == BAD and call(n=17, seed=65) == BAD      # a refusal comes first


def test_python_argument_errors():
    seed, pos = i64([1, 2, 3]), i32([5, 6, 7, 8])
    mixedgemm.uniform_rows(seed, pos)
    with pytest.raises(TypeError):
        mixedgemm.uniform_rows([1, 2, 3], pos)
    with pytest.raises(TypeError, match="seed"):
        mixedgemm.uniform_rows(seed.int(), pos)
    with pytest.raises(TypeError, match="pos"):
        mixedgemm.uniform_rows(seed, pos.long())
    with pytest.raises(RuntimeError, match="pos"):
        mixedgemm.uniform_rows(seed, pos.view(2, 2))
    with pytest.raises(TypeError, match="seed"):
        mixedgemm.uniform_rows(i64([1, 2, 3, 4, 5, 6])[::2], pos)
    with pytest.raises(RuntimeError, match="sub"):
        mixedgemm.uniform_rows(seed, pos, sub=i32([0, 1]))
    with pytest.raises(TypeError, match="sub"):
        mixedgemm.uniform_rows(seed, pos, sub=i64([0, 1, 2]))
    with pytest.raises(RuntimeError, match="row_seq"):
        mixedgemm.uniform_rows(seed, pos, row_seq=i32([0, 1, 2]))
    for n in (0, 17, -1, 2.0, True):
        with pytest.raises(ValueError, match="n"):
            mixedgemm.uniform_rows(seed, pos, n=n)
    for domain in (-1, 1 << 32, 0.5):
        with pytest.raises(ValueError, match="domain"):
            mixedgemm.uniform_rows(seed, pos, domain=domain)
    with pytest.raises(TypeError):
        mixedgemm.uniform_rows(seed, pos, 3)                                                   # n is keyword-only
    with pytest.raises(RuntimeError, match="out"):
        mixedgemm.uniform_rows(seed, pos, out=torch.zeros(3, 5))
    with pytest.raises(TypeError, match="out"):
        mixedgemm.uniform_rows(seed, pos, out=torch.zeros(3, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="out"):
        mixedgemm.uniform_rows(seed, pos, out=torch.zeros(4, 3).t())                          # unit stride along the rows
    with pytest.raises(RuntimeError, match="bits"):
        mixedgemm.uniform_rows(seed, pos, out=torch.zeros(3, 6)[:, :4], bits=torch.zeros(3, 4, dtype=torch.int32))      # another stride


# ---- the CPU path against the oracle -----------------------------------------------------------------------------------------------------
def test_the_cpu_path_gives_the_interface_vectors():
    for seed, pos, sub, domain, n, bits, u24 in INTERFACE_VECTORS:
        out, got = mixedgemm.uniform_rows(i64([seed]), i32([pos]), n=n, sub=i32([sub]), domain=domain, bits=True)
        assert out.dtype is torch.float32 and got.dtype is torch.int32 and out.shape == got.shape == (n, 1)
        assert got[:, 0].tolist() == [ro.as_int32(w) for w in bits]
        assert (out[:, 0].double() * 2 ** 24).tolist() == [float(w >> 8) for w in bits]


def check(seed, pos, n, sub, row_seq, domain, out, bits):
    want_u, want_bits = ro.uniform_rows(seed, pos, n, sub, row_seq, domain)
    assert out.dtype is torch.float32 and tuple(out.shape) == (n, len(pos))
    assert (out.double() * 2 ** 24).tolist() == [[float(x) for x in s] for s in want_u]
    if bits is not None:
        assert bits.tolist() == [[ro.as_int32(w) for w in s] for s in want_bits]


@pytest.mark.parametrize("case", range(6))
def test_uniform_rows_on_cpu_tensors_equals_the_oracle(case):
    rng = random.Random(case)
    for _ in range(8):
        batch, rows, n = rng.randrange(0, 6), rng.randrange(0, 12), rng.choice((1, 2, 3, 4, 5, 8, 15, 16))
        seed = [rng.choice((0, -1, 2 ** 63 - 1, -2 ** 63, rng.randrange(-2 ** 63, 2 ** 63))) for _ in range(batch)]
        pos = [rng.choice((0, -1, -2 ** 31, 2 ** 31 - 1, rng.randrange(0, 5000))) for _ in range(rows)]
        sub = [rng.choice((0, 1, -1, rng.randrange(-2 ** 31, 2 ** 31))) for _ in range(batch)] if case % 2 else None
        row_seq = [rng.randrange(-1, batch + 1) for _ in range(rows)] if case % 3 else None      # -1 and batch: outside
        domain = rng.choice((0, 0xFFFFFFFF, 7))
        given = dict(sub=None if sub is None else i32(sub), row_seq=None if row_seq is None else i32(row_seq))
        out = mixedgemm.uniform_rows(i64(seed), i32(pos), n=n, domain=domain, **given)
        check(seed, pos, n, sub, row_seq, domain, out, None)
        # into a view with slack, with the words: the slack stays
        ld = rows + rng.choice((0, 1, 3))
        store, wstore = torch.full((n, ld), -5.0), torch.full((n, ld), -5, dtype=torch.int32)
        got = mixedgemm.uniform_rows(i64(seed), i32(pos), n=n, domain=domain, out=store[:, :rows], bits=wstore[:, :rows], **given)
        assert rows == 0 or (got[0].data_ptr() == store.data_ptr() and got[1].data_ptr() == wstore.data_ptr())
        check(seed, pos, n, sub, row_seq, domain, got[0], got[1])
        assert bool((store[:, rows:] == -5.0).all()) and bool((wstore[:, rows:] == -5).all())
        assert torch.equal(got[0], out)
    # rows past the batch without row_seq are outside it
    out, bits = mixedgemm.uniform_rows(i64([11]), i32([4, 4, 4]), bits=True)
    assert out[:, 1:].abs().sum() == 0 and bits[:, 1:].abs().sum() == 0 and (bits[:, 0] != 0).all()


def test_what_separates_two_streams():
    """seed, sub, pos and domain each change every word; the same four give the same words in any batch and row"""
    base = dict(seed=5, pos=100, sub=0, domain=0)
    first = ro.words(n=16, **base)
    assert len(set(first)) == 16
    for name, other in (("seed", 5 + (1 << 32)), ("seed", 4), ("pos", 101), ("sub", 1), ("domain", 1)):
        changed = ro.words(n=16, **{**base, name: other})
        assert not set(changed) & set(first), name
    alone = mixedgemm.uniform_rows(i64([5]), i32([100]), n=16, bits=True)[1][:, 0]
    among = mixedgemm.uniform_rows(i64([9, 8, 5, 7]), i32([3, 100, 100, 2]), n=16, row_seq=i32([0, 2, 3, 1]), bits=True)[1]
    assert torch.equal(among[:, 1], alone) and alone.tolist() == [ro.as_int32(w) for w in first]
