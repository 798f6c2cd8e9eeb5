"""Every geometry of the far-offset and limit tests (tests/test_far_logits_gpu.py, tests/test_limits_gpu.py, tests/test_far_kv_gpu.py):
row distances, row counts, page counts, and the content of the rows.  The GPU tests import these and never restate a number;
tests/test_far_cpu.py proves by integer arithmetic which thresholds every row or page start crosses, where the offset lands when it is
computed in 32 bits, and how much device memory a case needs.

    B31, B32   2^31, 2^32 bytes:     where a signed / an unsigned 32-bit byte offset wraps
    E31, E32   2^31, 2^32 elements:  where `int row * int ld` / an unsigned element index wraps

A 32-bit wrap shows only if the data at the wrapped address gives another answer, so every row and page of a case has its own content
and the wrapped start of each lands in another row or page of the case, or in a guard band."""
import numpy as np

B31, B32, E31, E32 = 1 << 31, 1 << 32, 1 << 31, 1 << 32
GIB = 1 << 30
MEMORY_CAP = 20 * GIB                       # no test holds more device memory than this
CHUNK = 8192                                # MM_ARGMAX_CHUNK; tests/test_far_cpu.py holds it to the library's
MAX_VOCAB, MAX_ROWS = 1 << 20, 65535        # MM_ARGMAX_MAX_VOCAB, MM_ARGMAX_MAX_ROWS
NAN_BITS, NINF_BITS = 0x7FC0, 0xFF80


# ---- rows far apart in one buffer --------------------------------------------------------------------------------------------------
class FarRows:
    """`rows` rows of `width` elements of `itemsize` bytes, `ld` elements apart, the first at element `base` of its buffer, a guard
    band of `guard` elements before and after every row"""

    def __init__(self, name, base, ld, rows, width, guard, itemsize):
        self.name, self.base, self.ld, self.rows, self.width, self.guard, self.itemsize = name, base, ld, rows, width, guard, itemsize

    def start(self, r):
        """element index of row r's first element"""
        return self.base + r * self.ld

    def numel(self):
        """elements of the smallest buffer that holds every row and guard band"""
        return self.start(self.rows - 1) + self.width + self.guard

    def nbytes(self):
        return self.numel() * self.itemsize

    def crossed(self, r):
        """the thresholds that row r's start lies at or past"""
        e = self.start(r)
        return {n for n, at, v in (("B31", B31, e * self.itemsize), ("B32", B32, e * self.itemsize), ("E31", E31, e), ("E32", E32, e)) if v >= at}

    def locate(self, e):
        """where element index e of the buffer lies: ("row", r, column), ("guard", r) or None for memory the case does not fill"""
        for r in range(self.rows):
            if self.start(r) <= e < self.start(r) + self.width:
                return ("row", r, e - self.start(r))
            if self.start(r) - self.guard <= e < self.start(r) + self.width + self.guard:
                return ("guard", r)
        return None

    def wraps(self, r):
        """{what: element index} of row r's start computed in 32 bits, for every width that changes it: the element index and the byte
        offset, each modulo 2^32 (unsigned) and 2^31 (the low bits of a signed one)"""
        e, out = self.start(r), {}
        for name, value, unit in (("element", e, 1), ("byte", e * self.itemsize, self.itemsize)):
            for bits in (32, 31):
                w = value % (1 << bits)
                if w != value:
                    out[f"{name} mod 2^{bits}"] = w // unit
        return out


VOCAB = 2 * CHUNK + 5
GUARD = 64
LD = (1 << 29) + 24                          # 16-byte aligned rows: every entry point takes it (calib.accumulate needs ld % 8 == 0)
LD_ODD = (1 << 29) + 27                      # rows at every 2-byte alignment: argmax_rows, sample_rows, logprob_rows, process_logits
OUT_SHIFT = 32768                            # the second far view of the buffer starts this many elements after the first
FAR_IN = FarRows("far logits", GUARD, LD, 9, VOCAB, GUARD, 2)
FAR_OUT = FarRows("far out", GUARD + OUT_SHIFT, LD, 9, VOCAB, GUARD, 2)
FAR_ODD = FarRows("far logits, odd ld", GUARD, LD_ODD, 9, VOCAB, GUARD, 2)
LOGIT_VIEWS = (FAR_IN, FAR_OUT, FAR_ODD)
# an output view in a buffer of its own, so that one nine-row call of process_logits is accepted (input and output spans in one buffer
# meet); rows 2^28 + 24 apart keep it at 4 GiB: row 4 starts past B31, row 8 past B32 and E31
FAR_OUT_OWN = FarRows("far out, own buffer", GUARD, (1 << 28) + 24, 9, VOCAB, GUARD, 2)
LOGIT_BUFFER_ELEMENTS = max(v.numel() for v in LOGIT_VIEWS)
CALIB_K = 2 * CHUNK                          # the columns calib.accumulate reads of every far row (a multiple of 128)

# process_logits' token histories: [TOK_SEQS, LD_TOK] int32, LD_TOK the documented limit; the rows read sequences 0, 32 (which starts at
# B31 exactly) and 33 (past it)
LD_TOK = 1 << 24
TOK_SEQS = 34
TOKENS = FarRows("token histories", 0, LD_TOK, TOK_SEQS, 64, 0, 4)
ROW_SEQ = (33, 0, 32, 33, 5, 33, 32, -1, 33)           # the sequence of each of the nine rows; -1: no history
HIST_LEN = 48                                          # tokens filled (and at most read) per sequence

# process_logits' allowed_mask: int32 [9, LD_MASK], row 8 starts past B31
LD_MASK = (1 << 26) + 8
MASK = FarRows("allowed mask", 0, LD_MASK, 9, (VOCAB + 31) // 32, 0, 4)

PLANTED = (0, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 4, 777)     # each far row's own column


def bf16_bits(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def logit_rows(rows=9, vocab=VOCAB, seed=5, planted=PLANTED):
    """bf16 bits [rows, vocab]: Gaussian rows of standard deviation 3 (bf16 makes ties everywhere), every row different, the maximum of
    row r at its own column planted[r] and once more 13 columns later where the row goes on: the lowest index wins"""
    rng = np.random.default_rng(seed)
    bits = bf16_bits(rng.standard_normal((rows, vocab)) * 3.0)
    for r in range(rows):
        c = planted[r % len(planted)] % vocab
        bits[r, c] = 0x4220 + r                               # 40.0 and up: above every Gaussian value, different in every row
        if c + 13 < vocab:
            bits[r, c + 13] = bits[r, c]
    return bits


def sample_rows_bits(rows=9, vocab=VOCAB, planted=PLANTED):
    """the planted-column construction of tests/test_sample_gpu.py's check_places: all mass on one column, so every u draws it"""
    bits = np.empty((rows, vocab), dtype=np.uint16)
    bits[0::2], bits[1::2] = NINF_BITS, 0xC478                # -inf; -992.0: weight 0 next to 4.0
    for r in range(rows):
        bits[r, planted[r % len(planted)] % vocab] = 0x4080   # 4.0
    return bits


def integer_rows(rows, k, seed):
    """float32 [rows, k] of integers in -100 .. 100: exact in bf16 and fp16, every partial sum of |x| exact, every row different"""
    return np.random.default_rng(seed).integers(-100, 101, (rows, k)).astype(np.float32)


# ---- limits ------------------------------------------------------------------------------------------------------------------------
DISTINCT = 257                               # the row limit runs distinct[r % 257]
LIMIT_VOCABS = (8, CHUNK + 1)                # at rows = MAX_ROWS
VOCAB_PARTS = MAX_VOCAB // CHUNK             # 128
LIMIT_PLANTED = (0, 64 * CHUNK, 127 * CHUNK, MAX_VOCAB - 1)      # part 0, part 64, part 127, the last column
MAX_BIAS = 1 << 20
CALIB_MAX_ROWS, CALIB_MAX_K = 1 << 20, 32768
KV_MAX_B = 65535


# ---- paged KV pools just over 4 GiB ------------------------------------------------------------------------------------------------
class FarPool:
    """a paged cache [max_pages, L, 2, Hkv, P, row_bytes of data] whose data tensor is just over 4 GiB"""
    ROW_BYTES = {"int4": 64, "fp8": 128, "bf16": 256}

    def __init__(self, kind, L=2, Hkv=2, P=16):
        self.kind, self.L, self.Hkv, self.P = kind, L, Hkv, P
        self.itemsize = 2 if kind == "bf16" else 1
        self.page_bytes = L * 2 * Hkv * P * self.ROW_BYTES[kind]
        self.param_page_bytes = 0 if kind == "bf16" else L * 2 * Hkv * P * 4
        self.first_past_b31 = -(-B31 // self.page_bytes)     # the first page wholly past B31 (it starts there)
        self.first_past_b32 = -(-B32 // self.page_bytes)
        self.max_pages = self.first_past_b32 + 2
        self.last = self.max_pages - 1

    def far_pages(self):
        """the four kinds of page every page list mixes"""
        return [0, self.first_past_b31, self.first_past_b32, self.last]

    def pages(self):
        """the far pages and, so that a wrapped offset reads other content, the page each of them wraps to"""
        out = self.far_pages()
        for p in self.far_pages():
            for w in self.wraps(p).values():
                if w not in out:
                    out.append(w)
        return out

    def spare_pages(self):
        """pages no sequence holds, the destinations of kv_copy_pages: one below B31 and two past it"""
        return [2, self.first_past_b31 + 1, self.first_past_b31 + 2]

    def wraps(self, page):
        """{what: page} of the page's byte and element offsets modulo 2^32 and 2^31; every offset is a multiple of the page size"""
        out = {}
        for name, value, unit in (("byte", page * self.page_bytes, self.page_bytes),
                                  ("element", page * self.page_bytes // self.itemsize, self.page_bytes // self.itemsize)):
            for bits in (32, 31):
                w = value % (1 << bits)
                if w != value:
                    out[f"{name} mod 2^{bits}"] = w // unit
        return out

    def crossed(self, page):
        b = page * self.page_bytes
        return {n for n, at, v in (("B31", B31, b), ("B32", B32, b), ("E31", E31, b // self.itemsize), ("E32", E32, b // self.itemsize)) if v >= at}

    def data_bytes(self):
        return self.max_pages * self.page_bytes

    def param_bytes(self):
        return self.max_pages * self.param_page_bytes

    def twin_pages(self):
        return len(self.pages()) + len(self.spare_pages()) + 1

    def need_bytes(self):
        """the pool, its params, the twin, and 64 MiB for the operands"""
        return self.data_bytes() + self.param_bytes() + self.twin_pages() * (self.page_bytes + self.param_page_bytes) + (64 << 20)


POOLS = {kind: FarPool(kind) for kind in ("int4", "fp8", "bf16")}


def param_past_b31_pool_bytes(kind="int4"):
    """(param bytes, data bytes) of the smallest pool of `kind` whose fp16 param tensor itself passes B31: a row has 4 bytes of params
    for 64 (int4) or 128 (fp8) bytes of data, whatever L, Hkv and P are"""
    ratio = FarPool.ROW_BYTES[kind] // 4
    return B31, B31 * ratio


def logits_need_bytes():
    """the far logits buffer, the output buffer of its own, the token histories, the mask and 256 MiB for outputs, packed twins and
    workspaces; the far bias lists (bias_need_bytes) are held before these and released"""
    return LOGIT_BUFFER_ELEMENTS * 2 + FAR_OUT_OWN.nbytes() + TOKENS.nbytes() + MASK.nbytes() + (256 << 20)


def limits_need_bytes():
    """the largest case of tests/test_limits_gpu.py: MAX_ROWS rows of CHUNK + 1 logits, in and out, sample_rows' workspace (3 KiB per part
    and 2 KiB per row), and 256 MiB for the rest"""
    logits = MAX_ROWS * (CHUNK + 1) * 2
    return 2 * logits + MAX_ROWS * (2 * 3072 + 2048) + (256 << 20)


# ---- GEMM output, quantizer input and MoE rows past the thresholds -----------------------------------------------------------------
class FarMatrix:
    """a contiguous [rows, cols] matrix of `itemsize`-byte elements: which rows start at or past a threshold, and the rows to look at"""

    def __init__(self, name, rows, cols, itemsize):
        self.name, self.rows, self.cols, self.itemsize = name, rows, cols, itemsize

    def nbytes(self):
        return self.rows * self.cols * self.itemsize

    def first_row_past(self, threshold):
        """the first row that starts at or past B31 / B32 (bytes) or E31 / E32 (elements); None when the matrix ends before"""
        unit = self.cols * (self.itemsize if threshold[0] == "B" else 1)
        r = -(-{"B31": B31, "B32": B32, "E31": E31, "E32": E32}[threshold] // unit)
        return r if r < self.rows else None

    def crossed(self):
        return {t for t in ("B31", "B32", "E31", "E32") if self.first_row_past(t) is not None}

    def probe_rows(self):
        """the first row, the last row, and the row before and at every threshold the matrix crosses"""
        out = {0, self.rows - 1}
        for t in self.crossed():
            out |= {self.first_row_past(t) - 1, self.first_row_past(t)}
        return sorted(out)

    def wraps(self, r):
        """{what: row} of row r's offset modulo 2^32 and 2^31, in bytes and in elements, where that is a whole row"""
        out = {}
        for name, unit in (("byte", self.cols * self.itemsize), ("element", self.cols)):
            for bits in (32, 31):
                w = (r * unit) % (1 << bits)
                if w != r * unit and w % unit == 0:
                    out[f"{name} mod 2^{bits}"] = w // unit
        return out


GEMM_M, GEMM_N, GEMM_SPLIT = 66048, 65536, (128, 128, 128)
GEMM_CHUNK = 4096                            # rows per chunk of the device check: a multiple of the 128-row scale tile
GEMM_F32_M = 16640
GEMM_OUT = FarMatrix("matmul out, bf16", GEMM_M, GEMM_N, 2)
GEMM_OUT_F32 = FarMatrix("matmul out, fp32", GEMM_F32_M, GEMM_N, 4)

QUANT_ROWS, QUANT_K = 65664, 32768
QUANT_SPLITS = ((0, 0, 32768), (16384, 8192, 8192))
QUANT_CHUNK = 8192
QUANT_IN = FarMatrix("quantizer input, bf16", QUANT_ROWS, QUANT_K, 2)
QUANT_OUT_FP8 = FarMatrix("quantizer output, all fp8", QUANT_ROWS, QUANT_K, 1)

MOE_ROWS, MOE_H, MOE_TOP_K = 131080, 32768, 8
MOE_T = MOE_ROWS // MOE_TOP_K
MOE_X = FarMatrix("moe rows, bf16", MOE_ROWS, MOE_H, 2)


def moe_rows():
    """the rows moe_gather names and moe_combine's slots: the probe rows of the matrix and the rows their offsets wrap to"""
    return closure(MOE_X)


# activate_quantize_x: gate and up of the quantizers' shape, the smallest multiple of 128 rows at which a [rows, 32768] input passes E31.
# Row r holds row r % ACT_PERIOD of tests/act_exact_cases.py's lossless family; the period divides no distance a 32-bit offset wraps by
ACT_ROWS, ACT_K, ACT_PERIOD = QUANT_ROWS, QUANT_K, 509
ACT_IN = FarMatrix("activate_quantize_x gate / up, bf16", ACT_ROWS, ACT_K, 2)


def closure(matrix):
    """the probe rows of a matrix and the rows their 32-bit offsets wrap to: the rows a case fills and compares"""
    rows = set(matrix.probe_rows())
    for r in sorted(rows):
        rows |= set(matrix.wraps(r).values())
    return sorted(rows)


def gemm_group_bytes():
    """what each group of tests/test_far_gemm_gpu.py holds at once (its fixture is released before the next group's is made)"""
    return {"matmul": GEMM_OUT.nbytes() + GEMM_CHUNK * GEMM_N * 2 + (GEMM_M + GEMM_N) * 384 * 4,
            "quantizers": QUANT_IN.nbytes() + QUANT_ROWS * QUANT_K + QUANT_CHUNK * QUANT_K * 3,
            "activate": 2 * ACT_IN.nbytes() + ACT_ROWS * ACT_K + ACT_CHUNK_BYTES,
            "moe": MOE_X.nbytes() + MOE_T * MOE_H * 2}


ACT_CHUNK_BYTES = QUANT_CHUNK * ACT_K * 3


def gemm_need_bytes():
    """the largest group, with 512 MiB for operands and temporaries"""
    return max(gemm_group_bytes().values()) + (512 << 20)


# process_logits' bias lists: [BIAS.rows, 2^20] int32 and fp32, n_bias at its limit, so that rows start past B31, B32 and E31 (E32 would
# need 4096 rows, 32 GiB); only the rows of closure(BIAS) are filled, every other list is whatever torch.empty left
BIAS = FarMatrix("bias lists", 2056, MAX_BIAS, 4)
BIAS_VOCAB = 40


def bias_need_bytes():
    return 2 * BIAS.nbytes() + (256 << 20)
