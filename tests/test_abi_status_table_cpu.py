"""The statuses of the host layer, row by row: the decode GEMM entries, the gate/up decode entries, the RMSNorm quantizers (each family
one shared body in csrc/capi.hip), their `_supported` / `_supported_w` queries and the other entries that use the shared segment and
split helpers.  No device: every row fails a host check or has nothing to do (M == 0 / rows == 0 / N == 0), so it returns before any
launch -- the addresses are fakes that nothing may dereference.  The rows of the three grids carry a null output pointer as a
backstop: a row that passes every other check ends at that pointer's check, never at a launch.

EXPECTED holds what the library answered BEFORE the entries were folded into shared bodies (version 660), as literals: run this file
as a script (PYTHONPATH = the repository root) with MICROMIX_HIP_LIB pointing at the build to record, and it prints the dictionary.  A status of MM_ERR_LAUNCH (3) would
mean a row reached a launch: the recorder refuses to print it and the test refuses to run it."""
import itertools

from micromix_amd import _lib

A = 0x10000                  # fake addresses: A * i are 16-byte aligned, + 8 is not
X, R, S, NW, IDX, D, WS = A, 2 * A, 3 * A, 4 * A, 5 * A, 6 * A, 7 * A
BW, SFW = (8 * A, 9 * A, 10 * A), (11 * A, 12 * A, 13 * A)          # packed weights and their scales
O, SF = (14 * A, 15 * A, 16 * A), (17 * A, 18 * A, 19 * A)          # quantizer outputs and their scales
AX, SFA = (20 * A, 21 * A, 22 * A), (23 * A, 24 * A, 25 * A)        # quantized activations and their scales
EPS = 1e-5
ONCE, SPLIT_K, F32, NO_INT = _lib.MM_ROUND_ONCE, _lib.MM_SPLIT_K_ALWAYS, _lib.MM_OUT_F32, _lib.MM_NORM_NO_INTEGER_ROUND

MS = (-1, 0, 1, 9)
SPLITS = ((128, 0, 0), (100, 0, 0), (0, 0, 0), (-128, 128, 256))
WMODES = (0, 1, 7)
FLAGS = (0, ONCE, F32, SPLIT_K, NO_INT, 0x200)
DECODE = ("mm_qlinear_decode", "mm_rmsnorm_qlinear_decode", "mm_add_rmsnorm_qlinear_decode")
GATE_UP = ("mm_gate_up_activate_decode", "mm_rmsnorm_gate_up_activate_decode", "mm_add_rmsnorm_gate_up_activate_decode")
QUANT = ("mm_rmsnorm_quantize", "mm_add_rmsnorm_quantize")
WIDE = (4096, 0, 0)          # with I = 8192 the gate/up entries take their one-launch form (one 64-row workgroup per CU and more)


def head(variant, x=X, r=R, s=S, nw=NW):
    """the leading arguments that tell the three entries of a family apart: plain, norm, add + norm"""
    return ((x,), (x, nw, EPS), (x, r, s, nw, EPS))[variant]


def decode(variant, M=2, N=128, split=(128, 0, 0), wmode=1, flags=0, idx=IDX, B=BW, SFB=SFW, bias=None, d=D, **h):
    return (*head(variant, **h), idx, *B, *SFB, M, N, *split, wmode, flags, bias, d, None)


def gate_up(variant, M=2, I=128, split=(128, 0, 0), dsplit=(128, 0, 0), flags=0, idx=IDX, B=BW, SFB=SFW, o=O, sf=SF, ws=WS, ws_bytes=1 << 30, **h):
    return (*head(variant, **h), idx, *B, *SFB, M, I, *split, *dsplit, flags, *o, *sf, ws, ws_bytes, None)


def quant(variant, rows=2, K=128, split=(128, 0, 0), flags=0, idx=IDX, o=O, sf=SF, **h):
    return (*head(variant + 1, **h), rows, K, idx, *split, flags, *o, *sf, None)


def without(t, i):
    return tuple(None if j == i else p for j, p in enumerate(t))


def rows():
    """(entry, argument tuple) in a fixed order"""
    out = []
    add = lambda entry, args: out.append((entry, args))
    for v in range(3):
        # ---- the decode GEMM entries.  The grid, every row with D null
        for M, split, wmode, flags in itertools.product(MS, SPLITS, WMODES, FLAGS):
            add(DECODE[v], decode(v, M=M, split=split, wmode=wmode, flags=flags, d=None))
        add(DECODE[v], decode(v, N=0))
        add(DECODE[v], decode(v, N=-1))
        add(DECODE[v], decode(v, M=0, x=None, idx=None, B=(None,) * 3, SFB=(None,) * 3, d=None, nw=None, r=None, s=None))     # nothing to do
        add(DECODE[v], decode(v, M=9, x=None))                        # unsupported before the pointers
        add(DECODE[v], decode(v, split=(32768, 128, 0), x=None))      # K beyond 32768
        add(DECODE[v], decode(v, split=(8192, 128, 0), x=None))       # (beyond the norm's K)
        for kw in ({"x": None}, {"idx": None}, {"B": without(BW, 0)}, {"SFB": without(SFW, 0)}, {"split": (128, 128, 0), "B": without(BW, 1)},
                   {"split": (128, 0, 128), "SFB": without(SFW, 2)}):
            add(DECODE[v], decode(v, **kw))
        if v:
            for kw in ({"nw": None}, {"x": X + 8}, {"nw": NW + 8}):
                add(DECODE[v], decode(v, **kw))
        if v == 2:      # S_out equal to X, overlapping R by one row (M = 2 rows of 256 bytes), disjoint (D null: it would launch)
            for kw in ({"r": None}, {"s": None}, {"r": R + 8}, {"s": S + 8}, {"s": X}, {"s": R + 256}, {"s": R - 256}, {"s": R + 512, "d": None}):
                add(DECODE[v], decode(v, **kw))
        # ---- the gate/up decode entries.  The grid (the weight mode is not an argument), every row with oN null
        for M, split, flags in itertools.product(MS, SPLITS, FLAGS):
            add(GATE_UP[v], gate_up(v, M=M, split=split, flags=flags, o=without(O, 0)))
        for I, split in ((128, (128, 0, 0)), (8192, WIDE)):       # the two-launch and the one-launch form
            g = lambda **kw: add(GATE_UP[v], gate_up(v, I=I, split=split, dsplit=(I, 0, 0), **kw))
            g(M=0, x=None, idx=None, B=(None,) * 3, SFB=(None,) * 3, o=(None,) * 3, sf=(None,) * 3, ws=None, ws_bytes=0, nw=None, r=None, s=None)
            g(M=9, x=None)
            g(M=-1)
            for kw in ({"x": None}, {"idx": None}, {"B": without(BW, 0)}, {"SFB": without(SFW, 0)}, {"o": without(O, 0)}, {"sf": without(SF, 0)}):
                g(**kw)
            g(x=X + 8, ws=None)           # (the plain entry's two-launch form accepts the misaligned X: the null workspace ends it)
            if I == 128:                  # a null, a too small and a misaligned workspace: the two-launch form only
                g(ws=None)
                g(ws_bytes=2 * 256 * 2 - 1)
                g(ws=WS + 8)
            if v:
                g(nw=None)
                g(nw=NW + 8)
            if v == 2:
                for kw in ({"r": None}, {"s": None}, {"r": R + 8}, {"s": S + 8}, {"s": X}, {"s": R + 2 * split[0]}, {"s": R + 4 * split[0], "o": without(O, 0)}):
                    g(**kw)
        add(GATE_UP[v], gate_up(v, I=100, dsplit=(100, 0, 0)))
        add(GATE_UP[v], gate_up(v, I=256, dsplit=(128, 0, 0)))
        add(GATE_UP[v], gate_up(v, I=0, dsplit=(0, 0, 0)))
        add(GATE_UP[v], gate_up(v, I=-128, dsplit=(-128, 0, 0)))
        add(GATE_UP[v], gate_up(v, I=128, dsplit=(-128, 128, 128)))
    for v in range(2):
        # ---- the RMSNorm quantizers.  The grid (rows for M, the flag bits are not checked), every row with oN null
        for n, split, flags in itertools.product(MS, SPLITS, FLAGS):
            add(QUANT[v], quant(v, rows=n, split=split, flags=flags, o=without(O, 0)))
        add(QUANT[v], quant(v, K=256))
        add(QUANT[v], quant(v, K=32768 + 128, split=(32768 + 128, 0, 0)))
        add(QUANT[v], quant(v, rows=0, x=None, idx=None, o=(None,) * 3, sf=(None,) * 3, nw=None, r=None, s=None))
        for kw in ({"x": None}, {"nw": None}, {"idx": None}, {"o": without(O, 0)}, {"sf": without(SF, 0)},
                   {"K": 256, "split": (128, 128, 0), "o": without(O, 1)}, {"K": 256, "split": (128, 0, 128), "sf": without(SF, 2)}):
            add(QUANT[v], quant(v, **kw))
        add(QUANT[v], quant(v, x=X + 8, o=without(O, 0)))       # (the plain quantizer accepts these two: the null oN ends them)
        add(QUANT[v], quant(v, nw=NW + 8, o=without(O, 0)))
        if v:
            for kw in ({"r": None}, {"s": None}, {"x": X + 8}, {"nw": NW + 8}, {"r": R + 8}, {"s": S + 8}, {"s": X}, {"s": R + 256}, {"s": R - 256},
                       {"s": R + 512, "o": without(O, 0)}):
                add(QUANT[v], quant(v, **kw))
    # ---- the queries
    for M, N, split in itertools.product(MS, (0, 128, -1), SPLITS + ((32768, 128, 0), (8192, 128, 0), (128, 128, 128))):
        for q in ("mm_qlinear_decode_supported", "mm_rmsnorm_qlinear_decode_supported", "mm_down_activate_decode_supported"):
            add(q, (M, N, *split))
        for q, wmode in itertools.product(("mm_qlinear_decode_supported_w", "mm_rmsnorm_qlinear_decode_supported_w", "mm_down_activate_decode_supported_w"), WMODES):
            add(q, (M, N, *split, wmode))
    for M, I, split in itertools.product(MS + (2, 3, 4, 5), (0, 100, 128, 8192), SPLITS + (WIDE, (8192, 128, 0))):
        add("mm_gate_up_activate_decode_supported", (M, I, *split))
        add("mm_rmsnorm_gate_up_activate_decode_supported", (M, I, *split))
    # ---- the other entries that call the shared helpers: a null segment pointer, a bad split, nothing to do
    qargs = lambda o=O, sf=SF: (*o, *sf, None)
    for o, sf in ((without(O, 0), SF), (O, without(SF, 0))):
        add("mm_reorder_quantize", (X, 2, 128, IDX, 128, 0, 0, 0, *qargs(o, sf)))
        add("mm_reorder_quantize_gather", (X, 2, 256, IDX, 128, 0, 0, 0, *qargs(o, sf)))
        add("mm_activate_quantize", (X, R, 2, 128, 0, 0, *qargs(o, sf)))
        add("mm_downproj_quantize", (X, 2, 128, 0, 0, 0, *qargs(o, sf)))
        add("mm_gate_up_activate", (*itertools.chain(*zip(AX, BW)), *itertools.chain(*zip(SFA, SFW)), 2, 128, 128, 0, 0, 128, 0, 0, 0, *o, *sf, WS, 1 << 30, None))
    for a, b, sfa, sfb in ((without(AX, 0), BW, SFA, SFW), (AX, without(BW, 0), SFA, SFW), (AX, BW, without(SFA, 0), SFW), (AX, BW, SFA, without(SFW, 0))):
        inter = (*itertools.chain(*zip(a, b)), *itertools.chain(*zip(sfa, sfb)))
        add("mm_matmul", (*inter, 2, 128, 128, 0, 0, 1, 0, None, D, None))
        add("mm_matmul_ws", (*inter, 2, 128, 128, 0, 0, 1, 0, None, D, None, 0, None))
        add("mm_gate_up_activate", (*inter, 2, 128, 128, 0, 0, 128, 0, 0, 0, *O, *SF, WS, 1 << 30, None))
    add("mm_reorder_quantize", (X, 2, 128, IDX, 100, 28, 0, 0, *qargs()))
    add("mm_reorder_quantize", (None, 0, 128, None, 128, 0, 0, 0, *qargs((None,) * 3, (None,) * 3)))
    add("mm_activate_quantize", (X, R, 2, 0, 0, 0, *qargs()))
    add("mm_downproj_quantize", (X, 2, 128, -128, 128, 0, *qargs()))
    add("mm_gate_up_activate", (*[None] * 12, 0, 128, 128, 0, 0, 128, 0, 0, 0, *[None] * 6, None, 0, None))
    add("mm_gate_up_activate", (*[None] * 12, 2, 128, 0, 0, 0, 128, 0, 0, 0, *[None] * 6, None, 0, None))
    add("mm_gate_up_activate", (*[None] * 12, 2, 256, 128, 0, 0, 128, 0, 0, 0, *[None] * 6, None, 0, None))
    for split, B, SFB, gu in (((128, 0, 0), without(BW, 0), SFW, X), ((128, 0, 0), BW, without(SFW, 0), X), ((100, 0, 0), BW, SFW, X), ((0, 0, 0), BW, SFW, X),
                              ((-128, 128, 256), BW, SFW, X), ((128, 0, 0), BW, SFW, None), ((128, 0, 0), BW, SFW, X + 8)):
        add("mm_down_activate_decode", (gu, *B, *SFB, 2, 128, *split, 1, 0, None, D, None))
    add("mm_down_activate_decode", (None, *[None] * 6, 0, 128, 128, 0, 0, 1, 0, None, None, None))
    add("mm_down_activate_decode", (X, *BW, *SFW, 9, 128, 128, 0, 0, 1, 0, None, D, None))
    tab, offs = 26 * A, 27 * A
    for o, sf in ((without(O, 0), SF), (O, without(SF, 0))):
        add("mm_moe_quantize", (X, None, offs, tab, 2, 4, 4, 128, 128, 0, 0, 0, *o, *sf, None))
        add("mm_moe_activate_quantize", (X, R, offs, tab, 2, 4, 128, 128, 0, 0, *o, *sf, None, None))
    for a, sfa in ((without(AX, 0), SFA), (AX, without(SFA, 0))):
        add("mm_moe_matmul", (*a, *sfa, offs, tab, 2, 4, 4, 128, 128, 0, 0, 1, 0, D, None))
    return out


EXPECTED = {
    "mm_qlinear_decode": "222222222222222222222222222222222222222222222222222222222222222222222222004000004000222222111111111111111111111111111111111111222222222222222222224222224222222222111111111111111111111111111111111111222222222222222222444444444444222222111111111111111111111111111111111111222222222222222222020442222222",
    "mm_gate_up_activate_decode": "2222222222222222222222220022221111111111112222222222221111111111112222224422221111111111112222220422222222222042222222211121",
    "mm_rmsnorm_qlinear_decode": "222222222222222222222222222222222222222222222222222222222222222222222222002202002202222222111111111111111111111111111111111111222222222222222222222222222222222222111111111111111111111111111111111111222222222222222222442242442242222222111111111111111111111111111111111111222222222222222222020444222222222",
    "mm_rmsnorm_gate_up_activate_decode": "22222222222222222222222200220211111111111122222222222211111111111122222244224211111111111122222204222222222222204222222222211121",
    "mm_add_rmsnorm_qlinear_decode": "22222222222222222222222222222222222222222222222222222222222222222222222200220200220222222211111111111111111111111111111111111122222222222222222222222222222222222211111111111111111111111111111111111122222222222222222244224244224222222211111111111111111111111111111111111122222222222222222202044422222222222222222",
    "mm_add_rmsnorm_gate_up_activate_decode": "2222222222222222222222220022021111111111112222222222221111111111112222224422421111111111112222220422222222222222222222042222222222222222211121",
    "mm_rmsnorm_quantize": "222222111111111111111111000000111111111111111111222222111111111111111111222222111111111111111111120222222222",
    "mm_add_rmsnorm_quantize": "2222221111111111111111110000001111111111111111112222221111111111111111112222221111111111111111111202222222222222222222",
    "mm_qlinear_decode_supported": "000000000000000000000000000000000000000000200002220000220000000000000000000000000000",
    "mm_rmsnorm_qlinear_decode_supported": "000000000000000000000000000000000000000000100000120000020000000000000000000000000000",
    "mm_down_activate_decode_supported": "000000000000000000000000000000000000000000000000020002220000000000000000000000000000",
    "mm_qlinear_decode_supported_w": "000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000220000000000000220220220000000000000220220000000000000000000000000000000000000000000000000000000000000000000000000000000000000",
    "mm_rmsnorm_qlinear_decode_supported_w": "000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000110000000000000000110220000000000000000220000000000000000000000000000000000000000000000000000000000000000000000000000000000000",
    "mm_down_activate_decode_supported_w": "000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000220000000000220220220000000000000000000000000000000000000000000000000000000000000000000000000000000000000",
    "mm_gate_up_activate_decode_supported": "000000000000000000000000000000000000000000000000000000000000100011100021000000000000000000000000000000000000100011100021000000000000100011100011000000000000100011100011000000000000100011100011",
    "mm_rmsnorm_gate_up_activate_decode_supported": "000000000000000000000000000000000000000000000000000000000000100010100020000000000000000000000000000000000000100010100020000000000000100010100010000000000000100010100010000000000000100010100010",
    "mm_reorder_quantize": "2210",
    "mm_reorder_quantize_gather": "22",
    "mm_activate_quantize": "221",
    "mm_downproj_quantize": "221",
    "mm_gate_up_activate": "222222011",
    "mm_matmul": "2222",
    "mm_matmul_ws": "2222",
    "mm_down_activate_decode": "221122204",
    "mm_moe_quantize": "22",
    "mm_moe_activate_quantize": "22",
    "mm_moe_matmul": "22",
}


def record():
    lib, got = _lib.load(), {}
    for entry, args in rows():
        st = int(getattr(lib, entry)(*args))
        assert st != _lib.MM_ERR_LAUNCH or entry.endswith(("_supported", "_supported_w")), f"{entry}{args} reached a launch"
        got.setdefault(entry, []).append(st)
    return {entry: "".join(map(str, sts)) for entry, sts in got.items()}


def test_every_row_answers_what_version_660_answered():
    lib, seen = _lib.load(), {}
    assert lib.mm_version() == 660
    table = rows()
    assert {e for e, _ in table} == set(EXPECTED) and all(sum(e == n for e, _ in table) == len(s) for n, s in EXPECTED.items())
    for entry, args in table:
        i = seen[entry] = seen.get(entry, -1) + 1
        want = int(EXPECTED[entry][i])
        query = entry.endswith(("_supported", "_supported_w"))
        assert query or want != _lib.MM_ERR_LAUNCH, f"row {i} of {entry} is recorded as reaching a launch"
        got = int(getattr(lib, entry)(*args))
        assert got == want, f"row {i} of {entry}{args}: status {got}, version 660 before the shared bodies answered {want}"


if __name__ == "__main__":
    print("EXPECTED = {")
    for entry, s in record().items():
        print(f'    "{entry}": "{s}",')
    print("}")
