"""What the `mixedgemm` wrappers refuse, wrapper by wrapper: wrong dtype, CPU tensor, non-contiguous tensor, bad split, packed weight of
the wrong width, scale tensor one byte short, bad `rounding`, `out_sum` of the wrong shape -- each with the exception type and the
message the wrapper has always raised (the expressions are the message literals of mixedgemm.py before its repeated blocks became
helpers).  Every bad call raises before a launch.  One valid call per wrapper checks the shapes and dtypes that come back: a helper
that allocates the wrong width would show there.

The smallest shapes every wrapper takes: M = 2, K = 256 split (128, 128, 0), N = 128 (I = 128 for the gate/up forms), E = 2 experts and
n = 4 rows for the MoE pair."""
import pytest
import torch

from micromix_amd import mixedgemm as mg

pytestmark = pytest.mark.gpu

M, K, N, I, E, NROWS = 2, 256, 128, 128, 2, 4
SPLIT, DSPLIT = (128, 128, 0), (128, 0, 0)
EPS = 1e-5
BF, U8 = torch.bfloat16, torch.uint8
ROUNDING = (ValueError, r"rounding must be 'reference' or 'fused'")
SCALES_NAMED = (RuntimeError, r"SFBN holds \d+ scale bytes, needs at least \d+")
SCALES = (RuntimeError, r"weight scale tensors are too small")
GU_WEIGHT = (RuntimeError, r"B must be an interleaved fp4 gate/up weight \(interleave_gate_up\) whose split adds up to X's columns")
WIDTH = (RuntimeError, r"packed weights do not match \(KN, KS, KO\)")


def dtype_of(name):
    return (TypeError, rf"{name} must be torch\.bfloat16, got torch\.float32")


def cpu_of(name):
    return (RuntimeError, rf"{name} must be a device tensor \(HIP\); the MicroMix ops have no CPU path")


def contiguous_of(name):
    return (RuntimeError, rf"{name} must be contiguous")


def split_of(what):
    return (RuntimeError, rf"Value error in run_{what}: KN, KS, KO must be non-negative multiples of 128 that sum to K")


@pytest.fixture(scope="module")
def o(dev):
    """every operand, built once"""
    g = torch.Generator().manual_seed(5)
    rnd = lambda *shape: torch.randn(shape, generator=g).to(BF).to(dev)
    t = {"x": rnd(M, K), "r": rnd(M, K), "nw": rnd(K), "idx": torch.randperm(K, generator=g).to(torch.int16).to(dev), "gub": rnd(M, 2 * I),
         "src": rnd(NROWS, K), "offs": torch.tensor([0, 2, 4], dtype=torch.int32, device=dev)}
    t["x32"], t["xcpu"], t["xnc"] = t["x"].float(), t["x"].cpu(), rnd(M, 2 * K)[:, ::2]
    t["nw32"], t["nwshort"], t["srcnc"] = t["nw"].float(), t["nw"][:128], rnd(NROWS, 2 * K)[:, ::2]       # (the key "none" is absent: o.get gives None)
    t["b"] = mg.reorder_quantize_w4(rnd(N, K), t["idx"], *SPLIT)
    t["gu"] = mg.interleave_gate_up(mg.reorder_quantize_w4(rnd(I, K), t["idx"], *SPLIT), mg.reorder_quantize_w4(rnd(I, K), t["idx"], *SPLIT))
    t["down"] = mg.downproj_quantize_w4(rnd(N, I), *DSPLIT)
    t["qx"] = mg.reorder_quantize_x(t["x"], t["idx"], *SPLIT)
    t["table"] = mg.moe_expert_table([t["idx"]] * E, [t["b"]] * E, *SPLIT)
    t["qsrc"] = mg.moe_quantize(t["src"], None, t["offs"], t["table"])
    torch.cuda.synchronize()
    return t


def narrow(b):
    """the packed weight with BN four bytes narrower"""
    return (b[0][:, :-4].contiguous(), *b[1:])


def short(b):
    """the packed tuple with its first scale tensor one byte short of what its rows need (some quantizers allocate a tile more)"""
    need = (b[0].size(0) + 127) // 128 * 128 * (b[0].size(1) * 2 // 32)
    return (*b[:3], b[3][:need - 1], *b[4:])


def interleaved(a, b):
    return [t for pair in zip(a, b) for t in pair]


def quantized(rows, split=SPLIT):
    kn, ks, ko = split
    sf = lambda k: (rows // 128 + 1) * 128 * (k // 32)
    return [((rows, kn // 2), U8), ((rows, ks // 4 * 3), U8), ((rows, ko), U8), ((sf(kn),), U8), ((sf(ks),), U8), ((sf(ko),), U8)]


def moe_quantized():
    sf = lambda k: (NROWS // 128 + E) * 128 * (k // 32)
    return [((NROWS, 64), U8), ((NROWS, 96), U8), ((NROWS, 0), U8), ((sf(128),), U8), ((sf(128),), U8), ((0,), U8)]


# wrapper -> (the call, as a function of the operands and of the replacements a bad call makes; what a valid call returns; the bad calls)
def c_matmul(o, qx=None, b=None, **kw):
    return mg.matmul(*interleaved(qx or o["qx"], b or o["b"]), **kw)


def c_reorder_quantize_x(o, x="x", split=SPLIT):
    return mg.reorder_quantize_x(o[x], o["idx"], *split)


def c_activate_quantize_x(o, a="x", split=SPLIT):
    return mg.activate_quantize_x(o[a], o["r"], *split)


def c_rmsnorm_quantize_x(o, x="x", split=SPLIT, nw="nw", r="r"):
    return mg.rmsnorm_quantize_x(o[x], o.get(nw), EPS, o["idx"], *split)


def c_add_rmsnorm_quantize_x(o, x="x", split=SPLIT, out_sum=None, nw="nw", r="r"):
    return mg.add_rmsnorm_quantize_x(o[x], o.get(r), o.get(nw), EPS, o["idx"], *split, out_sum=out_sum)


def c_gate_up_activate(o, qx=None, gu=None, dsplit=DSPLIT, **kw):
    return mg.gate_up_activate(qx or o["qx"], gu or o["gu"], *dsplit, **kw)


def c_gate_up_activate_decode(o, x="x", gu=None, dsplit=DSPLIT, **kw):
    return mg.gate_up_activate_decode(o[x], o["idx"], gu or o["gu"], *dsplit, **kw)


def c_rmsnorm_gate_up_activate_decode(o, x="x", gu=None, dsplit=DSPLIT, nw="nw", **kw):
    return mg.rmsnorm_gate_up_activate_decode(o[x], o.get(nw), EPS, o["idx"], gu or o["gu"], *dsplit, **kw)


def c_add_rmsnorm_gate_up_activate_decode(o, x="x", gu=None, dsplit=DSPLIT, nw="nw", **kw):
    return mg.add_rmsnorm_gate_up_activate_decode(o[x], o["r"], o.get(nw), EPS, o["idx"], gu or o["gu"], *dsplit, **kw)


def c_down_activate_decode(o, gub="gub", down=None, dsplit=DSPLIT, **kw):
    return mg.down_activate_decode(o[gub] if isinstance(gub, str) else gub, down or o["down"], *dsplit, **kw)


def c_qlinear_decode(o, x="x", b=None, split=SPLIT, **kw):
    return mg.qlinear_decode(o[x], o["idx"], *(b or o["b"]), *split, **kw)


def c_rmsnorm_qlinear_decode(o, x="x", b=None, split=SPLIT, nw="nw", **kw):
    return mg.rmsnorm_qlinear_decode(o[x], o.get(nw), EPS, o["idx"], *(b or o["b"]), *split, **kw)


def c_add_rmsnorm_qlinear_decode(o, x="x", b=None, split=SPLIT, nw="nw", **kw):
    return mg.add_rmsnorm_qlinear_decode(o[x], o["r"], o.get(nw), EPS, o["idx"], *(b or o["b"]), *split, **kw)


def c_reorder_quantize_x_grouped(o, x="x", split=SPLIT):
    return mg.reorder_quantize_x_grouped([o[x], o["r"]], [o["idx"]] * 2, *split)[1]


def c_matmul_grouped(o, qx=None, b=None, **kw):
    return mg.matmul_grouped([o["qx"], qx or o["qx"]], [o["b"], b or o["b"]], **kw)[1]


def c_moe_quantize(o, src="src", **kw):
    return mg.moe_quantize(o[src] if isinstance(src, str) else src, None, o["offs"], o["table"], **kw)


def c_moe_activate_quantize(o, a="src", **kw):
    return mg.moe_activate_quantize(o[a] if isinstance(a, str) else a, o["src"], o["offs"], o["table"], **kw)


def c_moe_matmul(o, a=None, **kw):
    return mg.moe_matmul(a or o["qsrc"], o["offs"], o["table"], NROWS, **kw)


OUT = [((M, N), BF)]
SUM = [((M, K), BF)]
WRAPPERS = {
    c_matmul: (OUT, [
        ({"qx": "cpu"}, cpu_of("AN")), ({"b": "narrow"}, (RuntimeError, r"BN has shape \(128, 60\), expected \(128, 64\)")),
        ({"b": "short"}, SCALES_NAMED), ({"rounding": "bad"}, ROUNDING),
        ({"qx": "f32"}, (TypeError, r"AN must be torch\.uint8, got torch\.float32")), ({"qx": "nc"}, contiguous_of("AN"))]),
    c_reorder_quantize_x: (quantized(M), [
        ({"x": "x32"}, dtype_of("X")), ({"x": "xcpu"}, cpu_of("X")), ({"x": "xnc"}, contiguous_of("X")), ({"split": (128, 100, 28)}, split_of("reorder_quantize_x")),
        ({"split": (128, 0, 0)}, split_of("reorder_quantize_x"))]),
    c_activate_quantize_x: (quantized(M), [
        ({"a": "x32"}, dtype_of("input")), ({"a": "xcpu"}, cpu_of("input")), ({"a": "xnc"}, contiguous_of("input")),
        ({"split": (128, 100, 28)}, split_of("activate_quantize_x"))]),
    c_rmsnorm_quantize_x: (quantized(M), [
        ({"x": "x32"}, dtype_of("X")), ({"x": "xcpu"}, cpu_of("X")), ({"x": "xnc"}, contiguous_of("X")), ({"split": (128, 100, 28)}, split_of("rmsnorm_bf16_mixed")),
        ({"nw": "none"}, (TypeError, r"W must be a torch\.Tensor")), ({"nw": "nw32"}, dtype_of("W")), ({"nw": "nwshort"}, split_of("rmsnorm_bf16_mixed"))]),
    c_add_rmsnorm_quantize_x: (SUM + quantized(M), [
        ({"x": "x32"}, dtype_of("x")), ({"x": "xcpu"}, cpu_of("x")), ({"x": "xnc"}, contiguous_of("x")), ({"split": (128, 100, 28)}, split_of("rmsnorm_bf16_mixed")),
        ({"out_sum": "wrong"}, (RuntimeError, r"out_sum must be \[rows, K\]")), ({"r": "none"}, (TypeError, r"residual must be a torch\.Tensor")),
        ({"nw": "none"}, (TypeError, r"weight must be a torch\.Tensor")), ({"nw": "nw32"}, dtype_of("weight")), ({"nw": "nwshort"}, split_of("rmsnorm_bf16_mixed"))]),
    c_gate_up_activate: (quantized(M, DSPLIT), [
        ({"qx": "cpu"}, cpu_of("operand")), ({"dsplit": (100, 28, 0)}, split_of("activate_quantize_x")),
        ({"gu": "narrow"}, (RuntimeError, r"B must be an interleaved fp4 gate/up weight \(interleave_gate_up\) matching the activations' split")),
        ({"gu": "short"}, SCALES_NAMED), ({"rounding": "bad"}, ROUNDING)]),
    c_gate_up_activate_decode: (quantized(M, DSPLIT), [
        ({"x": "x32"}, dtype_of("X")), ({"x": "xcpu"}, cpu_of("X")), ({"x": "xnc"}, contiguous_of("X")), ({"dsplit": (100, 28, 0)}, split_of("activate_quantize_x")),
        ({"gu": "narrow"}, GU_WEIGHT), ({"gu": "short"}, SCALES_NAMED), ({"rounding": "bad"}, ROUNDING)]),
    c_rmsnorm_gate_up_activate_decode: (quantized(M, DSPLIT), [
        ({"x": "x32"}, dtype_of("X")), ({"x": "xcpu"}, cpu_of("X")), ({"x": "xnc"}, contiguous_of("X")), ({"dsplit": (100, 28, 0)}, split_of("activate_quantize_x")),
        ({"gu": "narrow"}, GU_WEIGHT), ({"gu": "short"}, SCALES_NAMED), ({"rounding": "bad"}, ROUNDING),
        ({"nw": "none"}, (AttributeError, r"'NoneType' object has no attribute 'dtype'")), ({"nw": "nw32"}, dtype_of("norm_weight")), ({"nw": "nwshort"}, GU_WEIGHT)]),
    c_add_rmsnorm_gate_up_activate_decode: (SUM + quantized(M, DSPLIT), [
        ({"x": "x32"}, dtype_of("X")), ({"x": "xcpu"}, cpu_of("X")), ({"x": "xnc"}, contiguous_of("X")), ({"dsplit": (100, 28, 0)}, split_of("activate_quantize_x")),
        ({"gu": "narrow"}, GU_WEIGHT), ({"gu": "short"}, SCALES_NAMED), ({"rounding": "bad"}, ROUNDING),
        ({"out_sum": "wrong"}, (RuntimeError, r"out_sum must have X's shape")),
        ({"nw": "none"}, (AttributeError, r"'NoneType' object has no attribute 'dtype'")), ({"nw": "nw32"}, dtype_of("norm_weight")), ({"nw": "nwshort"}, GU_WEIGHT)]),
    c_down_activate_decode: (OUT, [
        ({"gub": "x32"}, dtype_of("GU")), ({"gub": "xcpu"}, cpu_of("GU")), ({"gub": "xnc"}, contiguous_of("GU")), ({"dsplit": (100, 28, 0)}, split_of("activate_quantize_x")),
        ({"down": "narrow"}, (RuntimeError, r"packed weights do not match \(DN, DS, DO\)")), ({"down": "short"}, SCALES), ({"rounding": "bad"}, ROUNDING)]),
    c_qlinear_decode: (OUT, [
        ({"x": "x32"}, dtype_of("X")), ({"x": "xcpu"}, cpu_of("X")), ({"x": "xnc"}, contiguous_of("X")), ({"split": (128, 0, 0)}, split_of("reorder_quantize_x")),
        ({"b": "narrow"}, WIDTH), ({"b": "short"}, SCALES), ({"rounding": "bad"}, ROUNDING)]),
    c_rmsnorm_qlinear_decode: (OUT, [
        ({"x": "x32"}, dtype_of("X")), ({"x": "xcpu"}, cpu_of("X")), ({"x": "xnc"}, contiguous_of("X")), ({"split": (128, 0, 0)}, split_of("rmsnorm_quantize_x")),
        ({"b": "narrow"}, WIDTH), ({"b": "short"}, SCALES), ({"rounding": "bad"}, ROUNDING),
        ({"nw": "none"}, (AttributeError, r"'NoneType' object has no attribute 'dtype'")), ({"nw": "nw32"}, dtype_of("norm_weight")), ({"nw": "nwshort"}, split_of("rmsnorm_quantize_x"))]),
    c_add_rmsnorm_qlinear_decode: (SUM + OUT, [        # (it looks at the residual first: against a CPU X that is the tensor out of place)
        ({"x": "x32"}, dtype_of("X")), ({"x": "xcpu"}, (RuntimeError, r"residual is on cuda:0, expected cpu")), ({"x": "xnc"}, contiguous_of("X")), ({"split": (128, 0, 0)}, split_of("rmsnorm_quantize_x")),
        ({"b": "narrow"}, WIDTH), ({"b": "short"}, SCALES), ({"rounding": "bad"}, ROUNDING), ({"out_sum": "wrong"}, (RuntimeError, r"out_sum must have X's shape")),
        ({"nw": "none"}, (AttributeError, r"'NoneType' object has no attribute 'dtype'")), ({"nw": "nw32"}, dtype_of("norm_weight")), ({"nw": "nwshort"}, split_of("rmsnorm_quantize_x"))]),
    c_reorder_quantize_x_grouped: (quantized(M), [
        ({"x": "x32"}, (TypeError, r"X\[0\] must be torch\.bfloat16, got torch\.float32")), ({"x": "xnc"}, contiguous_of(r"X\[0\]")),
        ({"split": (128, 100, 28)}, split_of("reorder_quantize_x"))]),
    c_matmul_grouped: (OUT, [
        ({"qx": "cpu"}, cpu_of("group 1 operand")), ({"b": "narrow"}, (RuntimeError, r"group 1: packed weights do not match N / split / weight mode of group 0")),
        ({"b": "short"}, (RuntimeError, r"group 1: a scale tensor is too small")), ({"rounding": "bad"}, ROUNDING),
        ({"qx": "nc"}, contiguous_of("group 1 operand"))]),
    c_moe_quantize: (moe_quantized(), [
        ({"src": "x32n"}, dtype_of("src")), ({"src": "cpun"}, cpu_of("src")), ({"src": "ncn"}, contiguous_of("src")), ({"mode": "w"}, (ValueError, r"mode must be 'x' or 'w4'")),
        ({"out": "narrow"}, (RuntimeError, r"packed output must be \[4, 64\], got \[4, 60\]")),
        ({"out": "short"}, (RuntimeError, r"a scale output is smaller than moe_sf_bytes\(n, E, Kseg\)"))]),
    c_moe_activate_quantize: (moe_quantized(), [
        ({"a": "x32n"}, dtype_of("a")), ({"a": "cpun"}, cpu_of("a")), ({"a": "ncn"}, contiguous_of("a")), ({"out": "narrow"}, (RuntimeError, r"packed output must be \[4, 64\], got \[4, 60\]")),
        ({"out": "short"}, (RuntimeError, r"a scale output is smaller than moe_sf_bytes\(n, E, Kseg\)"))]),
    c_moe_matmul: ([((NROWS, N), BF)], [
        ({"rounding": "bad"}, ROUNDING), ({"a": "cpu4"}, cpu_of("activation segment")), ({"a": "nc4"}, contiguous_of("activation segment")),
        ({"a": "narrow"}, (RuntimeError, r"activation segment must be \[4, 64\], got \[4, 60\]")),
        ({"a": "short"}, (RuntimeError, r"an activation scale tensor is smaller than moe_sf_bytes\(n, E, Kseg\)")),
        ({"out": "wrongout"}, (RuntimeError, r"out must be \[4, 128\], got \[5, 128\]"))]),
}
SOURCE = {c_matmul: "b", c_gate_up_activate: "gu", c_gate_up_activate_decode: "gu", c_rmsnorm_gate_up_activate_decode: "gu",
          c_add_rmsnorm_gate_up_activate_decode: "gu", c_down_activate_decode: "down", c_qlinear_decode: "b", c_rmsnorm_qlinear_decode: "b",
          c_add_rmsnorm_qlinear_decode: "b", c_matmul_grouped: "b", c_moe_quantize: "qsrc", c_moe_activate_quantize: "qsrc", c_moe_matmul: "qsrc"}


def resolve(call, o, kw):
    """the words of the table as operands: a packed tuple narrowed / shortened / on the CPU, a wrong out_sum, the MoE sources"""
    out = {}
    for k, v in kw.items():
        if v == "narrow":
            v = narrow(o[SOURCE[call]])
        elif v == "short":
            v = short(o[SOURCE[call]])
        elif v == "cpu":
            v = tuple(t.cpu() for t in o["qx"])
        elif v == "wrong":
            v = torch.empty((M + 1, K), dtype=BF, device=o["x"].device)
        elif v == "f32":
            v = (o["qx"][0].float(), *o["qx"][1:])
        elif v == "nc":
            v = (torch.zeros((M, 2 * SPLIT[0] // 2), dtype=U8, device=o["x"].device)[:, ::2], *o["qx"][1:])
        elif v == "cpu4":
            v = tuple(t.cpu() for t in o["qsrc"])
        elif v == "nc4":
            v = (torch.zeros((NROWS, 2 * SPLIT[0] // 2), dtype=U8, device=o["x"].device)[:, ::2], *o["qsrc"][1:])
        elif v == "wrongout":
            v = torch.empty((NROWS + 1, N), dtype=BF, device=o["x"].device)
        elif v == "ncn":
            v = o["srcnc"]
        elif v == "x32n":
            v = o["src"].float()
        elif v == "cpun":
            v = o["src"].cpu()
        out[k] = v
    return out


@pytest.mark.parametrize("call", list(WRAPPERS), ids=lambda c: c.__name__[2:])
def test_wrapper_refuses_and_returns(o, call):
    want, bad = WRAPPERS[call]
    for kw, (exc, match) in bad:
        with pytest.raises(exc, match=match):
            call(o, **resolve(call, o, kw))
    got = call(o)
    torch.cuda.synchronize()
    got = [got] if isinstance(got, torch.Tensor) else list(got)
    assert [(tuple(t.shape), t.dtype) for t in got] == want, call.__name__
