"""The geometry of tests/far_cases.py proved by integer arithmetic, without a GPU: which of B31 / B32 (2^31, 2^32 bytes) and E31 / E32
(2^31, 2^32 elements) every row or page start crosses, that every case crosses what its GPU test claims, where the start lands when it
is computed in 32 bits (it has to be another row or page of the case, with other content, or a guard band), and the device memory a
case needs.  Run with -s for the tables.  A constant changed so that a case no longer crosses a threshold fails here."""
import numpy as np

from micromix_amd import _lib
import far_cases as fc
import kv_verify_oracle as vo


def table(title, lines):
    print(f"\n{title}")
    for line in lines:
        print("   ", line)


def test_the_constants_are_the_library_s():
    assert fc.CHUNK == _lib.MM_ARGMAX_CHUNK and fc.MAX_ROWS == _lib.MM_ARGMAX_MAX_ROWS and fc.MAX_VOCAB == _lib.MM_ARGMAX_MAX_VOCAB
    assert fc.VOCAB == 2 * _lib.MM_ARGMAX_CHUNK + 5 and fc.VOCAB_PARTS == 128 and fc.MAX_VOCAB % fc.CHUNK == 0
    assert [c // fc.CHUNK for c in fc.LIMIT_PLANTED] == [0, 64, 127, 127] and fc.LIMIT_PLANTED[-1] == fc.MAX_VOCAB - 1
    assert fc.LD_TOK == 1 << 24 and fc.MAX_BIAS == 1 << 20 and fc.CALIB_MAX_ROWS == 1 << 20 and fc.CALIB_MAX_K == 32768 and fc.KV_MAX_B == 65535
    assert fc.LIMIT_VOCABS == (8, fc.CHUNK + 1) and fc.DISTINCT == 257


def wrap_lines(view, content=None):
    """the table of a FarRows, after asserting that every wrapped start lands in another row (whose content there differs) or in a guard"""
    lines = []
    for r in range(view.rows):
        wraps = view.wraps(r)
        assert bool(wraps) == bool(view.crossed(r)), (view.name, r)
        shown = []
        for what, e in wraps.items():
            where = view.locate(e)
            assert where is not None, f"{view.name} row {r}: {what} = element {e} lands in memory the case does not fill"
            if where[0] == "row":
                _, other, col = where
                assert other != r, (view.name, r, what)
                if content is not None:                      # what a read of row r at the wrapped address would see, where it is filled
                    n = view.width - col
                    assert not np.array_equal(content[other, col:], content[r, :n]), (view.name, r, what)
            shown.append(f"{what} -> {where}")
        lines.append(f"row {r}: element {view.start(r)}, byte {view.start(r) * view.itemsize}, crosses {sorted(view.crossed(r)) or '-'}; "
                     + "; ".join(shown))
    return lines


def test_far_logit_rows_cross_every_threshold_and_wrap_onto_other_content():
    bits = fc.logit_rows()
    assert len({bits[r].tobytes() for r in range(9)}) == 9
    for view in fc.LOGIT_VIEWS:
        assert view.rows == 9 and view.width == fc.VOCAB and view.guard == 64
        assert "B31" in view.crossed(2) and not view.crossed(1)                                  # row 2 starts past B31
        assert {"E31", "B32"} <= view.crossed(4) and "E31" not in view.crossed(3)               # row 4 past E31 and B32
        assert view.crossed(8) == {"B31", "B32", "E31", "E32"} and "E32" not in view.crossed(7)  # row 8 past E32
        table(f"{view.name}: ld {view.ld}, {view.nbytes() / fc.GIB:.3f} GiB", wrap_lines(view, bits))
    own = fc.FAR_OUT_OWN
    assert own.crossed(4) == {"B31"} and not own.crossed(3) and own.crossed(8) == {"B31", "B32", "E31"} and "B32" not in own.crossed(7)
    table(f"{own.name}: ld {own.ld}, {own.nbytes() / fc.GIB:.3f} GiB", wrap_lines(own, bits))
    assert fc.LD == 2 ** 29 + 24 and fc.LD_ODD == 2 ** 29 + 27
    assert fc.LD % 8 == 0 and fc.FAR_IN.base % 8 == 0 and fc.CALIB_K % 128 == 0 and fc.CALIB_K <= fc.VOCAB     # calib.accumulate's alignment
    assert {fc.FAR_ODD.start(r) % 8 for r in range(9)} == set(range(8))                          # rows at every 2-byte alignment
    # the two views of process_logits do not meet: a row of one lies in the gap of the other
    assert fc.FAR_IN.width + 2 * fc.GUARD <= fc.OUT_SHIFT and fc.FAR_OUT.start(0) - fc.FAR_IN.start(0) == fc.OUT_SHIFT < fc.LD - fc.VOCAB - fc.GUARD
    assert fc.LOGIT_BUFFER_ELEMENTS * 2 < 8.1 * fc.GIB
    # the planted columns are each row's own, in every part of the vocabulary and on both sides of each part boundary
    assert len(set(fc.PLANTED)) == 9 and {c // fc.CHUNK for c in fc.PLANTED} == {0, 1, 2}
    assert vo.argmax_rows(fc.logit_rows()).tolist() == list(fc.PLANTED)
    s = fc.sample_rows_bits()
    assert [(s[r] == 0x4080).nonzero()[0].tolist() for r in range(9)] == [[c] for c in fc.PLANTED]


def test_token_histories_and_mask_rows_pass_b31():
    t = fc.TOKENS
    assert t.ld == fc.LD_TOK and not t.crossed(31) and t.crossed(32) == {"B31"} and t.start(32) * 4 == fc.B31 and t.crossed(33) == {"B31"}
    used = sorted(set(s for s in fc.ROW_SEQ if s >= 0))
    assert {32, 33} <= set(used) and max(used) < fc.TOK_SEQS and len(fc.ROW_SEQ) == 9 and fc.HIST_LEN <= t.width
    # a 32-bit byte offset of sequence 32 / 33 is that of sequence 0 / 1 (2^31 bytes lower): both are filled, with other tokens
    for s in (32, 33):
        assert t.wraps(s) == {"byte mod 2^31": t.start(s - 32)} and t.locate(t.start(s - 32)) == ("row", s - 32, 0)
    m = fc.MASK
    assert m.width == (fc.VOCAB + 31) // 32 and m.crossed(8) == {"B31"} and not m.crossed(7)
    assert m.locate(m.wraps(8)["byte mod 2^31"])[:2] == ("row", 0)
    table("process_logits operands", [f"tokens [{t.rows}, {t.ld}] int32: {t.nbytes() / fc.GIB:.3f} GiB, sequences 32 and 33 start at / past B31",
                                      f"allowed_mask [9, {m.ld}] int32: {m.nbytes() / fc.GIB:.3f} GiB, row 8 starts past B31"])


def test_bias_lists_pass_b31_b32_and_e31():
    """bias_idx / bias_val are [rows, n_bias] with n_bias <= 2^20 as their row distance, so far rows take many rows of the longest list"""
    b = fc.BIAS
    assert b.cols == fc.MAX_BIAS and b.crossed() == {"B31", "B32", "E31"} and b.first_row_past("E32") is None
    assert (b.first_row_past("B31"), b.first_row_past("B32"), b.first_row_past("E31")) == (512, 1024, 2048) and b.rows <= fc.MAX_ROWS
    rows = fc.closure(b)
    assert set(b.probe_rows()) <= set(rows) and all(w in rows and w != r for r in rows for w in b.wraps(r).values())
    assert 2 * b.nbytes() > 16 * fc.GIB and fc.bias_need_bytes() < fc.MEMORY_CAP
    table("process_logits bias lists", [f"bias_idx, bias_val [{b.rows}, {b.cols}]: {b.nbytes() / fc.GIB:.3f} GiB each, need "
                                        f"{fc.bias_need_bytes() / fc.GIB:.2f} GiB; rows filled and compared {rows}; wraps "
                                        + "; ".join(f"row {r} -> {b.wraps(r)}" for r in rows if b.wraps(r))])


def test_kv_pools_cross_b31_and_b32_and_wrap_onto_pages_of_the_case():
    lines = []
    for kind, pool in fc.POOLS.items():
        far = pool.far_pages()
        assert far[0] == 0 and far[3] == pool.max_pages - 1 and len(set(pool.pages())) == len(pool.pages())
        assert fc.B32 < pool.data_bytes() <= fc.B32 + 4 * pool.page_bytes                       # just over 4 GiB
        assert pool.crossed(far[1]) >= {"B31"} and not pool.crossed(far[1] - 1) >= {"B31"}       # the first page wholly past B31
        assert pool.crossed(far[2]) >= {"B31", "B32"} and "B32" not in pool.crossed(far[2] - 1)
        assert pool.crossed(far[3]) >= {"B31", "B32"} and far[3] > far[2]
        assert "E31" in pool.crossed(far[2]) and ("E32" in pool.crossed(far[3])) == (kind != "bf16")   # bf16: 4 GiB is 2^31 elements
        for p in far:
            for what, w in pool.wraps(p).items():
                assert w in pool.pages() and w != p, (kind, p, what)
        # the params of the int4 and fp8 pools cross nothing at this size
        assert pool.param_bytes() < fc.B31
        lines.append(f"{kind}: {pool.max_pages} pages of {pool.page_bytes} bytes, data {pool.data_bytes() / fc.GIB:.4f} GiB, params "
                     f"{pool.param_bytes() / fc.GIB:.4f} GiB; pages {pool.pages()}; "
                     + "; ".join(f"page {p} crosses {sorted(pool.crossed(p)) or '-'} wraps {pool.wraps(p) or '-'}" for p in far))
    table("paged KV pools", lines)


def test_a_pool_whose_params_pass_b31_does_not_fit_the_memory_cap():
    """a pool whose fp16 param tensor itself passes B31 cannot be built within MEMORY_CAP: whatever L, Hkv and P are, int4 data is 16 times
    its params and fp8 data 32 times"""
    for kind, ratio in (("int4", 16), ("fp8", 32)):
        param, data = fc.param_past_b31_pool_bytes(kind)
        assert param == fc.B31 and data == ratio * fc.B31 and data > fc.MEMORY_CAP
        pool = fc.POOLS[kind]
        assert pool.page_bytes == ratio * pool.param_page_bytes


def test_every_case_fits_the_memory_cap():
    needs = {"test_far_logits_gpu": fc.logits_need_bytes(), "test_far_logits_gpu, bias lists": fc.bias_need_bytes(),
             "test_limits_gpu": fc.limits_need_bytes()}
    needs.update({f"test_far_kv_gpu[{k}]": p.need_bytes() for k, p in fc.POOLS.items()})
    table("device memory needed", [f"{k}: {v / fc.GIB:.2f} GiB" for k, v in needs.items()])
    assert all(v < fc.MEMORY_CAP for v in needs.values())
    assert fc.logits_need_bytes() > 8 * fc.GIB and all(p.need_bytes() > 4 * fc.GIB for p in fc.POOLS.values())


def test_gemm_quantizer_and_moe_matrices_cross_their_thresholds():
    lines = []
    for m, want in ((fc.GEMM_OUT, {"B31", "B32", "E31", "E32"}), (fc.GEMM_OUT_F32, {"B31", "B32"}), (fc.QUANT_IN, {"B31", "B32", "E31"}),
                    (fc.QUANT_OUT_FP8, {"B31", "E31"}), (fc.ACT_IN, {"B31", "B32", "E31"}), (fc.MOE_X, {"B31", "B32", "E31", "E32"})):
        assert m.crossed() == want, (m.name, m.crossed())
        probes = m.probe_rows()
        assert probes[0] == 0 and probes[-1] == m.rows - 1
        for t in want:
            r = m.first_row_past(t)
            assert 0 < r < m.rows and {r - 1, r} <= set(probes)
        lines.append(f"{m.name} [{m.rows}, {m.cols}]: {m.nbytes() / fc.GIB:.3f} GiB, first row past "
                     + ", ".join(f"{t}: {m.first_row_past(t)}" for t in sorted(want)) + f"; probe rows {probes}; wraps "
                     + "; ".join(f"row {r} -> {m.wraps(r)}" for r in probes if m.wraps(r)))
    table("GEMM, quantizer and MoE matrices", lines)
    assert fc.GEMM_M % 128 == 0 and fc.GEMM_CHUNK % 128 == 0 and fc.GEMM_F32_M % 128 == 0 and sum(fc.GEMM_SPLIT) == 384
    assert fc.QUANT_ROWS % 128 == 0 and fc.QUANT_CHUNK % 128 == 0 and all(sum(s) == fc.QUANT_K for s in fc.QUANT_SPLITS)
    assert fc.MOE_T == 16385 and fc.MOE_T * fc.MOE_TOP_K == fc.MOE_ROWS
    # every row a wrapped offset of a MoE probe row lands on is itself one of the rows of the case (each has its own content)
    rows = fc.moe_rows()
    assert all(w in rows and w != r for r in rows for w in fc.MOE_X.wraps(r).values()) and len(rows) < 32
    # GEMM and quantizers compute every row from every operand row, so a wrapped output offset overwrites another row of the output:
    # the whole output is compared with the chunked run
    # activate_quantize_x: the smallest multiple of 128 rows whose input passes E31, and a period of the row content that no wrap hides
    assert fc.ACT_ROWS % 128 == 0 and (fc.ACT_ROWS - 128) * fc.ACT_K <= fc.E31 < fc.ACT_ROWS * fc.ACT_K
    assert all(w % fc.ACT_PERIOD != r % fc.ACT_PERIOD for r in fc.ACT_IN.probe_rows() for w in fc.ACT_IN.wraps(r).values())
    groups = fc.gemm_group_bytes()
    assert fc.gemm_need_bytes() == max(groups.values()) + (512 << 20) < fc.MEMORY_CAP
    table("device memory needed", [f"test_far_gemm_gpu: {fc.gemm_need_bytes() / fc.GIB:.2f} GiB, the largest of "
                                   + ", ".join(f"{k} {v / fc.GIB:.2f}" for k, v in groups.items())])
