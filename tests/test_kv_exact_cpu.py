"""CPU proofs of the preconditions tests/test_kv_exact_gpu.py relies on, from the oracles alone (tests/kv_oracle.py,
kv_prefill_oracle.py): the value grids survive the int4 cache bit for bit, the needle code book leaves 40 nats, the targets cover every
edge, the oracles return the constructed answers within the stated bounds, and the int4 rule's edge rows quantize to pinned bytes."""
import numpy as np
import pytest

from micromix_amd import _lib
import kv_exact_cases as kc
import kv_oracle as ko
import kv_prefill_oracle as kpo


def host_cache(kind, c, lens=None, poison=False, L=2, layer=1, seed=0):
    """append a builder's K / V to a host cache image with the oracle; returns (data, param, (indptr, indices, last))"""
    lens = c["lens"] if lens is None else lens
    indptr, indices, last, max_pages = kc.page_table(lens, c["P"], seed)
    data, param = kc.empty_host_cache(kind, max_pages, L, c["Hkv"], c["P"], poison)
    ko.append(data, param, indptr, indices, last, kc.bf16_bits(c["K"]), kc.bf16_bits(c["V"]), kc.indptr_of(lens), layer)
    return data, param, (indptr, indices, last)


def cached_values(kind, c, lens=None):
    data, param, tbl = host_cache(kind, c, lens)
    out = [ko.dequantized(data, param, *tbl, 1, b) for b in range(len(tbl[2]))]
    K = np.concatenate([k.transpose(1, 0, 2) for k, _ in out])
    V = np.concatenate([v.transpose(1, 0, 2) for _, v in out])
    return K, V


BUILDERS = {
    "needle_prefill": lambda: kc.needle_prefill_case(4),
    "needle_decode": lambda: kc.needle_decode_case(2),
    "ramp_prefill": lambda: kc.ramp_prefill(3, 2, 24, 1.0),
    "ramp_decode": lambda: kc.ramp_decode(4, 2, 16, 1.0, lengths=[1, 33, 4097]),
    "count_prefill": lambda: kc.count_prefill(*kc.COUNT_PREFILL_CASES[2]),
    "count_decode": lambda: kc.count_decode(7, 2, 24),
}


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_int4_cache_holds_the_grids_exactly(name):
    """V of every builder, and the integer K of ramp / count, come back from the int4 cache bit for bit; the needle's +-1 K comes back
    as the two values the margin argument assumes"""
    c = BUILDERS[name]()
    lens = c["lens"] if "N" not in c else [c["N"]]
    K4, V4 = cached_values("int4", c, lens)
    K16, V16 = cached_values("bf16", c, lens)
    assert np.array_equal(K16, c["K"].astype(np.float64)) and np.array_equal(V16, c["V"].astype(np.float64))
    assert np.array_equal(V4, V16)
    if name.startswith("needle"):
        hi, lo = 15 * 0.13330078125 - 1.06640625, -1.06640625               # fp16(2 / 15), base 8: codes 15 / 0
        assert np.array_equal(K4, np.where(c["K"] > 0, hi, lo))
        assert abs(hi - 0.9331) < 1e-4 and abs((hi - lo) / 2 - 0.99975) < 1e-4
    else:
        assert np.array_equal(K4, K16)


def test_v_grid_on_1000_random_rows():
    rng = np.random.default_rng(0)
    rows = rng.integers(-8, 8, (1000, 128)).astype(np.float32) / 8
    rows[:, 0], rows[:, 1] = -1.0, 0.875
    rows = rng.permuted(rows, axis=1)
    codes, s, z = ko.quantize_row(rows)
    assert (s == np.float16(0.125)).all() and (z == np.float16(1.0)).all()
    assert np.array_equal(codes.astype(np.float32) * 0.125 - 1.0, rows)
    k = rng.integers(0, 16, (1000, 128)).astype(np.float32)
    k[:, 4], k[:, 5] = 0.0, 15.0
    codes, s, z = ko.quantize_row(k)
    assert (s == np.float16(1.0)).all() and (z.view(np.uint16) == 0).all() and np.array_equal(codes.astype(np.float32), k)


def test_v_grid_rows_differ_and_decode():
    pos = np.array([0, 1, 2, 31, 32, 4095, 4096, 32767])
    v = kc.v_grid(3, pos[:, None], np.arange(4)[None, :]).reshape(-1, 128)
    assert v.min() == -1.0 and v.max() == 0.875 and np.array_equal(v * 8, np.round(v * 8))
    diff = (v[:, None, :] != v[None, :, :]).sum(-1)
    assert (diff[~np.eye(len(v), dtype=bool)] >= 5).all()
    assert kc.v_decode(kc.v_grid(3, 4097, 2)) == "seq 3 pos 4097 head 2"
    assert (kc.v_grid(1, pos, 0)[:, 112:] == 0).all()


def test_needle_margin_is_40_nats():
    """from the code books: the worst off-target correlation of 32768 codes per kv head"""
    for h in range(4):
        assert kc.worst_correlation(h, kc.MAX_POS) <= 71              # (128 - 71) * 8 * 0.9997 / sqrt(128) = 40.3
    assert kc.needle_margin_nats(4, kc.MAX_POS) >= kc.MARGIN_NATS
    assert np.exp(-kc.MARGIN_NATS) * kc.MAX_POS < 1e-12                # all other tokens together
    # and on a dequantized int4 cache: the actual score lead of a target over every other token
    c = kc.needle_decode_case(2)
    K4, _ = cached_values("int4", c, [c["N"]])
    for b in (0, 7):
        for hq in range(c["Hq"]):
            s = K4[:, hq // c["g"]] @ c["q"][b, hq].astype(np.float64) / np.sqrt(128)
            t = c["targets"][b, hq]
            assert s[t] - np.delete(s, t).max() >= kc.MARGIN_NATS


@pytest.mark.parametrize("i", range(len(kc.NEEDLE_PREFILL_SHAPES)))
def test_needle_prefill_targets_cover_every_edge(i):
    c = kc.needle_prefill_case(i)
    bq = 64 // c["g"]
    assert c["new"][:5] == [0, 1, bq - 1, bq, bq + 1] and c["new"][5] > 2 * bq and c["new"][6] > 2 * bq
    assert kc.needle_prefill_uncovered(c) == []
    # the check itself bites: hide one edge
    edge = next(e for e in kc.edge_positions(max(c["lens"]) - 1, c["P"]) if 0 < e < 250)
    broken = dict(c, targets=np.where(c["targets"] == edge, 0, c["targets"]))
    assert edge in kc.needle_prefill_uncovered(broken)


def test_needle_shapes_cover_every_g_and_page_size():
    assert sorted(s[0] for s in kc.NEEDLE_PREFILL_SHAPES) == sorted(kc.G_VALUES)
    assert {s[2] for s in kc.NEEDLE_PREFILL_SHAPES} == set(kc.PAGE_SIZES) == {s[2] for s in kc.NEEDLE_DECODE_SHAPES}
    assert set(kc.NEEDLE_DECODE_SHAPES[0][3]) == {1, 31, 32, 33, 4096, 32768}
    assert {c[2] for c in kc.COUNT_PREFILL_CASES} == set(kc.PAGE_SIZES) == {c[2] for c in kc.COUNT_DECODE_SHAPES}


def test_needle_32k_and_decode_targets_cover_every_edge():
    c = kc.needle_prefill_32k()
    assert c["lens"] == [32768] and kc.needle_prefill_uncovered(c) == []
    assert len(kc.edge_positions(32767, 16)) == 2 * 2047 + 1
    for i in range(len(kc.NEEDLE_DECODE_SHAPES)):
        d = kc.needle_decode_case(i)
        assert kc.needle_decode_uncovered(d) == []
        assert set(d["lens"]) == set(d["lengths"])


@pytest.mark.parametrize("kind", ["int4", "bf16"])
@pytest.mark.parametrize("i", [0, 3, 5, 8])
def test_needle_prefill_oracle_returns_the_targets(kind, i):
    c = kc.needle_prefill_case(i)
    data, param, tbl = host_cache(kind, c)
    got = kpo.attention(kc.bf16_bits(c["q"]), data, param, *tbl, kc.indptr_of(c["new"]), 1)
    assert np.abs(got - c["expect"]).max() <= 1e-12


@pytest.mark.parametrize("kind", ["int4", "bf16"])
def test_needle_decode_oracle_returns_the_targets(kind):
    c = kc.needle_decode_case(2)
    pages = kc.page_table([c["N"]], c["P"], 0)[1]
    data, param, _ = host_cache(kind, c, [c["N"]])
    tbl = kc.prefix_table(pages, c["P"], c["lens"])
    got = ko.attention(kc.bf16_bits(c["q"]), data, param, *tbl, 1)
    assert np.abs(got - c["expect"]).max() <= 1e-12


@pytest.mark.parametrize("kind", ["int4", "bf16"])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_ramp_oracle_returns_own_position_or_position_0(kind, sign):
    c = kc.ramp_prefill(5, 2, 24, sign)
    data, param, tbl = host_cache(kind, c)
    got = kpo.attention(kc.bf16_bits(c["q"]), data, param, *tbl, kc.indptr_of(c["new"]), 1)
    assert np.abs(got - c["expect"]).max() <= 1e-12
    d = kc.ramp_decode(4, 2, 16, sign, lengths=[1, 2, 33, 4097])
    pages = kc.page_table([d["N"]], 16, 0)[1]
    data, param, _ = host_cache(kind, d, [d["N"]])
    got = ko.attention(kc.bf16_bits(d["q"]), data, param, *kc.prefix_table(pages, 16, d["lens"]), 1)
    assert np.abs(got - d["expect"]).max() <= 1e-12


def test_ramp_scores_are_exact_in_fp32():
    q = kc.ramp_q()
    assert np.array_equal(kc.to_bf16(q), q)
    t = np.array([0, 1, 15, 16, 255, 4096, 32767])
    s = (kc.ramp_k(t) * q).sum(-1, dtype=np.float32)
    assert np.array_equal(s, (512 * t).astype(np.float32)) and 512 * 32767 < 2 ** 24
    assert 512 / np.sqrt(128) > 45.0
    # the ramp priors: one inside a kv tile, the others on every multiple of 64 (chunk lengths are multiples of 64), and the
    # library splits these shapes
    assert any(a % 64 for a in kc.RAMP_PRIORS) and {a for a in kc.RAMP_PRIORS if a % 64 == 0} == set(range(0, 1281, 64))
    for g in kc.G_VALUES:
        c = kc.ramp_prefill(g, 2, 16, 1.0)
        assert _lib.load().mm_paged_prefill_workspace_bytes(c["q"].shape[0], len(c["new"]), c["Hq"], 2, max(c["lens"])) > 0
        assert all(n == 3 * (64 // g) + 1 for n in c["new"]) and max(c["lens"]) > 1280


@pytest.mark.parametrize("kind", ["int4", "bf16"])
def test_count_oracle_returns_the_mean(kind):
    c = kc.count_prefill(*kc.COUNT_PREFILL_CASES[2])
    data, param, tbl = host_cache(kind, c)
    got = kpo.attention(kc.bf16_bits(c["q"]), data, param, *tbl, kc.indptr_of(c["new"]), 1)
    assert np.abs(got - c["expect"]).max() <= 1e-13
    # one lost token at 4096 moves its dimension by 8 ulps: far outside the 1-ulp bound
    want = kc.count_expect(4095)
    assert (1.875 / 4096) / kc.bf16_ulp(want)[0] >= 4.0
    assert kc.bf16_ulp(np.array([0.0, 1.0, 1.875, 0.49]))[0] == 0 and kc.bf16_ulp(1.0) == 2.0 ** -7


# name -> (the code of every distinct value of the row, in ascending order of value; scale bits; zero bits): literals, from the
# rule by hand (s = fp16(max(range, 1e-5) / 15), base = clamp(rint(-min / s)), code = clamp(rint(x / s) + base), zero = fp16(base s))
EDGE_EXPECT = {
    "zeros": ([0], 0x000B, 0x0000),                    # fp16(1e-5 / 15) = 11 * 2^-24, a subnormal
    "const_pos": ([15], 0x000B, 0x0000),
    "const_neg": ([0], 0x000B, 0x00A5),                # base 15: zero = 165 * 2^-24
    "offset_pos": ([15] * 17, 0x2C44, 0x0000),         # the 17 bf16 values of linspace(10, 11)
    "offset_neg": ([0] * 17, 0x2C44, 0x3C00),
    "halves": ([0, 2, 2, 4, 4, 6, 6, 8, 8, 10, 10, 12, 12, 14, 14, 15], 0x3C00, 0x4800),   # rint(-7.5 .. 7.5) + 8, the top one clips
    "tiny_range": ([0, 3, 6, 9, 12], 0x000B, 0x0000),  # 0, 2e-6 .. 8e-6 over s = 6.56e-7
    "tiny_single": ([0, 0], 0x000B, 0x0000),           # 1e-7 / s = 0.15
    "bf16_max": ([0, 15], 0x7BFF, 0x7BFF),
    "outlier": ([0, 15], 0x6133, 0x0000),
    "neg_zero": ([0, 2, 5, 7, 10, 12, 15], 0x34CD, 0x0000),   # 0, 0.75 .. 4.5 over s = 0.30005
    "neg_zero_only": ([0], 0x000B, 0x0000),
    "subnormal": ([0, 0, 0, 0], 0x000B, 0x0000),
    # 62 bf16 values of linspace(-2, 1) and 4 subnormals over s = fp16(0.1984), base 10
    "subnormal_mixed": ([0, 0, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 6, 6, 6, 6, 6, 7, 7, 7, 7, 8, 8, 8, 8, 9, 9, 9, 9,
                         10, 10, 10, 10, 10, 10, 11, 11, 11, 11, 11, 12, 12, 12, 12, 13, 13, 13, 13, 14, 14, 14, 14, 15, 15, 15],
                        0x325A, 0x3FF0),
}


def test_edge_rows_quantize_to_pinned_bytes():
    rows = kc.edge_rows()
    assert set(rows) == set(EDGE_EXPECT)
    for name, row in rows.items():
        assert np.isfinite(row).all() and np.array_equal(kc.to_bf16(row), row), name
        with np.errstate(over="ignore"):
            codes, s, z = ko.quantize_row(row)
        assert np.isfinite(s.astype(np.float32)) and np.isfinite(z.astype(np.float32)), name
        assert not (z.view(np.uint16) & 0x8000), f"{name}: zero must not carry a sign"
        want_codes, want_s, want_z = EDGE_EXPECT[name]
        vals, inverse = np.unique(row, return_inverse=True)            # -0.0 and 0.0 are one value
        assert len(vals) == len(want_codes), name
        assert np.array_equal(codes, np.array(want_codes, dtype=np.uint8)[inverse]), name      # every element of the row
        assert (int(s.view(np.uint16)), int(z.view(np.uint16))) == (want_s, want_z), name
    # in the mixed row the subnormals themselves sit on the base code
    assert set(ko.quantize_row(rows["subnormal_mixed"])[0][0::2].tolist()) == {10}
    # the zero parameter of a row whose minimum is 0 is +0.0
    assert ko.quantize_row(np.zeros(128))[2].view(np.uint16) == 0


def test_edge_batch_holds_every_row_as_k_and_v():
    k, v = kc.edge_batch(4, 1)
    for name, row in kc.edge_rows().items():
        for src in (k, v):
            assert (src.reshape(-1, 128).view(np.uint32) == row.view(np.uint32)).all(-1).any(), name
    assert np.isfinite(k).all() and np.isfinite(v).all()
    # poisoned images: NaN everywhere until appended
    d4, p4 = kc.empty_host_cache("int4", 2, 1, 1, 2, True)
    d16, _ = kc.empty_host_cache("bf16", 2, 1, 1, 2, True)
    assert (d4 == 0xFF).all() and np.isnan(p4.astype(np.float32)).all() and np.isnan(ko.bf16_to_f32(d16)).all()
    assert 0 not in kc.page_table([40, 3], 16, 5)[1]
