"""GPU tests of mixedgemm.moe_activate_quantize and of SparseMoEBlock(capturable=True, fused_activation=True):

  1. exact: with h_out given, the six outputs are byte for byte moe_quantize(h_out, None, offsets, table) -- packed bytes everywhere,
     scale bytes where an expert's rows put them -- at one lane quad (K 128), all three segments (K 384), K 1 024, the 1024-thread
     variant (K 14 336, n 16), per-expert random reorder indices, experts empty at the front / middle / end, all rows in one expert,
     M_e at 127 / 128 / 129, E = 64 with n = 8;
  2. untouched: outputs and h_out pre-filled with 0xFF keep every byte that no expert owns, after junk offsets and from offsets[E] on;
  3. bounds: every operand at the end of an allocation of its own (tests/moe_activate_bounds_probe.py, a child process);
  4. budgeted: h_out against the fp64 oracle and against torch's F.silu(a) * b (tests/moe_act_oracle.py: fewer than 1e-3 differing
     elements, none more than 3 bf16 ulps off), every finite bf16 as `a` within 1 ulp, non-finite inputs confined to their rows, and the
     quantized outputs against the oracle's quantizer of the oracle's h within tests/test_direct_quantize_gpu.py's budget;
  5. the block: bit-equal to the chain composed here from the public ops with h_out in the middle, router logits the default block's,
     the same eight calls into the library at E = 8 and E = 64 and none of the capturable block's two torch launches (ten launches
     become eight); one capture at T = 16 replayed on other routings.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import moe_act_oracle as ma
import moe_block_oracle as mb
from conftest import bits_from_t, t_from_bits, u8
from micromix_amd import _lib, mixedgemm
from model_case import gen_bf16, gen_index
from oracle import mx_oracle as o

pytestmark = pytest.mark.gpu
FMTS = ("fp4", "fp6", "fp8")


def index_table(dev, E, split, seed, identity=False):
    """a device table whose experts have reorder indices of their own (all the quantizer reads) and share zero weights of 16 features"""
    import torch
    K, N = sum(split), 16
    idx = [torch.arange(K, dtype=torch.int16, device=dev) if identity else gen_index(dev, K, seed + e) for e in range(E)]
    z = lambda *s: torch.zeros(s, dtype=torch.uint8, device=dev)
    B = (z(N, split[0] // 2), z(N, split[1] // 2), z(N, split[2] // 2), z(128 * split[0] // 32), z(128 * split[1] // 32), z(128 * split[2] // 32))
    return idx, mixedgemm.moe_expert_table(idx, [B] * E, *split)


def filled(dev, n, E, split):
    import torch
    widths = (split[0] // 2, split[1] // 4 * 3, split[2])
    return tuple(torch.full((n, w), 0xFF, dtype=torch.uint8, device=dev) for w in widths) + \
        tuple(torch.full((mixedgemm.moe_sf_bytes(n, E, k),), 0xFF, dtype=torch.uint8, device=dev) for k in split)


def filled_h(dev, n, K):
    import torch
    return torch.full((n, K), -1, dtype=torch.int16, device=dev).view(torch.bfloat16)


def offsets_of(counts, dev):
    import torch
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return off.tolist(), torch.from_numpy(off).to(dev)


def sf_run(sf, off, e, kseg):
    """expert e's run of a packed scale tensor: tile off[e] // 128 + e, ceil(M / 128) tiles"""
    tile = 128 * kseg // 32
    return sf[(off[e] // 128 + e) * tile:][: (off[e + 1] - off[e] + 127) // 128 * tile]


def assert_same_quantization(got, want, off, split, label):
    """two 6-tuples (host arrays) that started from the same fill: packed bytes equal everywhere, scale bytes at the valid offsets of
    every expert's run"""
    for i, kseg in enumerate(split):
        if kseg == 0:
            continue
        assert np.array_equal(got[i], want[i]), f"{label}: packed segment {i}"
        for e in range(len(off) - 1):
            valid = o.sf_valid_offsets(off[e + 1] - off[e], kseg)
            assert np.array_equal(sf_run(got[3 + i], off, e, kseg)[valid], sf_run(want[3 + i], off, e, kseg)[valid]), f"{label}: scales of segment {i}, expert {e}"


def ab_on(dev, n, K, seed):
    a, b = ma.draw_ab(n, K, seed)
    return a, b, t_from_bits(a, dev), t_from_bits(b, dev)


# ---- 1. the quantization part, exact --------------------------------------------------------------------------------------------------
SHAPES = {"one quad": (128, (0, 128, 0)), "three segments": (384, (128, 128, 128)), "K 1024": (1024, (512, 128, 384))}
OFFSETS = {
    "empty front middle end": (0, 5, 0, 0, 7, 3, 0, 0),
    "all in one expert": (0, 0, 0, 20, 0, 0, 0, 0),
    "127 128 129": (127, 128, 129, 0, 129, 128, 127, 1),
    "E 64 n 8": tuple(1 if e in (3, 9, 17, 26, 31, 40, 57, 63) else 0 for e in range(64)),
}
EXACT = [(s, c) for s in SHAPES for c in OFFSETS] + [("1024 threads", "n 16")]


@pytest.mark.parametrize("shape,case", EXACT)
def test_quantization_is_moe_quantize_of_h_out_byte_for_byte(dev, shape, case):
    import torch
    K, split = SHAPES.get(shape, (14336, (12288, 1024, 1024)))
    counts = OFFSETS.get(case, (0, 5, 0, 0, 8, 3, 0, 0))
    E, n = len(counts), sum(counts)
    assert (K, n) != (14336, 0) and (shape != "1024 threads" or n == 16)
    off, offsets = offsets_of(counts, dev)
    idx, table = index_table(dev, E, split, seed=40 + K)
    assert not torch.equal(idx[0], idx[-1]) and not torch.equal(idx[0], torch.arange(K, dtype=torch.int16, device=dev))
    _, _, a, b = ab_on(dev, n, K, seed=K + n)
    h = filled_h(dev, n, K)
    got = mixedgemm.moe_activate_quantize(a, b, offsets, table, out=filled(dev, n, E, split), h_out=h)
    want = mixedgemm.moe_quantize(h, None, offsets, table, out=filled(dev, n, E, split))
    again = mixedgemm.moe_activate_quantize(a, b, offsets, table, out=filled(dev, n, E, split))          # without h_out: the same bytes
    torch.cuda.synchronize()
    assert not (bits_from_t(h) == 0xFFFF).all(axis=1).any(), "a row of h_out was not written"
    assert_same_quantization([u8(t) for t in got], [u8(t) for t in want], off, split, f"{shape}, {case}")
    assert_same_quantization([u8(t) for t in again], [u8(t) for t in want], off, split, f"{shape}, {case}, h_out=None")
    first = next(i for i in range(3) if split[i])
    assert (u8(got[first]) != 0xFF).any()


# ---- 2. what no expert owns -----------------------------------------------------------------------------------------------------------
def test_outputs_no_expert_owns_stay_as_they_were(dev):
    import torch
    K, split, E = 384, (128, 128, 128), 8
    counts = (0, 5, 0, 0, 7, 3, 0, 0)
    owned, n = sum(counts), sum(counts) + 6                   # six slots from offsets[E] on belong to nobody
    off, offsets = offsets_of(counts, dev)
    _, table = index_table(dev, E, split, seed=70)
    _, _, a, b = ab_on(dev, n, K, seed=71)
    h = filled_h(dev, n, K)
    got = [u8(t) for t in mixedgemm.moe_activate_quantize(a, b, offsets, table, out=filled(dev, n, E, split), h_out=h)]
    want = [u8(t) for t in mixedgemm.moe_quantize(h[:owned].clone(), None, offsets, table, n=owned, out=filled(dev, owned, E, split))]
    hb = bits_from_t(h)
    assert (hb[owned:] == 0xFFFF).all() and not (hb[:owned] == 0xFFFF).all(axis=1).any()
    for i, kseg in enumerate(split):
        assert np.array_equal(got[i][:owned], want[i]) and (got[i][owned:] == 0xFF).all(), f"packed segment {i}"
        mine = np.full_like(got[3 + i], 0xFF)
        for e in range(E):
            valid = o.sf_valid_offsets(off[e + 1] - off[e], kseg)
            sf_run(mine, off, e, kseg)[valid] = sf_run(want[3 + i], off, e, kseg)[valid]
        assert np.array_equal(got[3 + i], mine), f"a scale byte of segment {i} that no expert owns was written"
    # offsets that are no plan's: decreasing, negative, past n -- nothing may be written at all, h_out included
    for junk in ([5, 3] + [n + 9] * (E - 1), [-4] * (E + 1), [n + 1] * (E + 1)):
        h = filled_h(dev, n, K)
        out = mixedgemm.moe_activate_quantize(a, b, torch.tensor(junk, dtype=torch.int32, device=dev), table, out=filled(dev, n, E, split), h_out=h)
        torch.cuda.synchronize()
        assert all((u8(t) == 0xFF).all() for t in out) and (bits_from_t(h) == 0xFFFF).all(), junk


# ---- 3. operands at the end of their allocations ----------------------------------------------------------------------------------------
def test_activate_quantize_stays_inside_its_operands():
    """tests/moe_activate_bounds_probe.py in a child process (a memory fault would kill it, not this run)"""
    probe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "moe_activate_bounds_probe.py")
    r = subprocess.run([sys.executable, probe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"the probe died (exit {r.returncode}):\n{r.stdout}\n{r.stderr[-2000:]}"
    lines = [l.split() for l in r.stdout.splitlines() if l.startswith("case")]
    assert len(lines) == 4 and "done" in r.stdout, r.stdout
    for _, label, got, want in lines:
        assert got == want, f"{label}: other bytes with the operands at the end of their allocations"


# ---- 4. the activation part, budgeted -------------------------------------------------------------------------------------------------
def split_rows(rows):
    """rows per expert of the budgeted cases: an empty expert, one of a single row"""
    return (rows // 3, 0, rows - rows // 3 - 1, 1)


@pytest.fixture(scope="module")
def budget_runs(dev):
    """per BUDGET_CASES entry, computed once: inputs, the oracle's h, the device's h_out and six outputs (host arrays)"""
    import torch
    cache = {}

    def get(i):
        if i not in cache:
            rows, K, split, seed = ma.BUDGET_CASES[i]
            counts = split_rows(rows)
            off, offsets = offsets_of(counts, dev)
            idx, table = index_table(dev, len(counts), split, seed=90 + i)
            a_bits, b_bits, a, b = ab_on(dev, rows, K, seed)
            h = filled_h(dev, rows, K)
            q = mixedgemm.moe_activate_quantize(a, b, offsets, table, out=filled(dev, rows, len(counts), split), h_out=h)
            torch_h = torch.nn.functional.silu(a) * b
            torch.cuda.synchronize()
            cache[i] = dict(off=off, idx=[u8(t) for t in idx], a=a_bits, b=b_bits, want=ma.h_oracle(a_bits, b_bits), h=bits_from_t(h),
                            torch_h=bits_from_t(torch_h), q=[u8(t) for t in q], split=split)
        return cache[i]
    return get


@pytest.mark.parametrize("i", range(len(ma.BUDGET_CASES)))
def test_h_out_is_within_the_budget_of_the_fp64_oracle(budget_runs, i):
    r = budget_runs(i)
    ma.assert_within_budget(r["h"], r["want"], f"h_out against the oracle, case {ma.BUDGET_CASES[i][:2]}")


@pytest.mark.parametrize("i", range(len(ma.BUDGET_CASES)))
def test_h_out_is_within_the_budget_of_torch_silu_mul(budget_runs, i):
    r = budget_runs(i)
    ma.assert_within_budget(r["h"], r["torch_h"], f"h_out against torch's F.silu(a) * b, case {ma.BUDGET_CASES[i][:2]}")


@pytest.mark.parametrize("i", range(len(ma.BUDGET_CASES)))
def test_quantized_outputs_close_to_the_oracles_quantizer_of_the_oracles_h(budget_runs, i):
    """tests/test_direct_quantize_gpu.py's budget as it stands, per expert"""
    r = budget_runs(i)
    off, split = r["off"], r["split"]
    for e in range(len(off) - 1):
        M = off[e + 1] - off[e]
        if M == 0:
            continue
        want = o.reorder_quantize(r["want"][off[e]:off[e + 1]], r["idx"][e], *split, "x")
        for s in range(3):
            if not split[s]:
                continue
            got_p, got_sf = r["q"][s][off[e]:off[e + 1]], sf_run(r["q"][3 + s], off, e, split[s])
            offs = o.sf_valid_offsets(M, split[s])
            assert got_p.shape == want[s].shape
            packed_diff, sf_diff = float((got_p != want[s]).mean()), float((got_sf[offs] != want[3 + s][offs]).mean())
            print(f"case {i} expert {e} segment {s}: {packed_diff:.2e} of the packed bytes, {sf_diff:.2e} of the scale bytes differ")
            assert sf_diff < 1e-3 and packed_diff < 1e-3, (i, e, s)
            dg = o.dequant_segment(got_p, got_sf, M, split[s], FMTS[s])
            dw = o.dequant_segment(want[s], want[3 + s], M, split[s], FMTS[s])
            amax = np.abs(dw).reshape(M, -1, 32).max(-1, keepdims=True)
            step = amax * 2.0 ** (-o.FORMATS[FMTS[s]]["mbits"])
            assert np.all(np.abs(dg - dw).reshape(M, -1, 32) <= step + 1e-30), (i, e, s)


def test_every_finite_bf16_is_within_one_ulp(dev):
    import torch
    a_bits = ma.all_finite_bf16()
    b_bits = np.full_like(a_bits, 0x3F80)
    n, K, split = 512, 128, (0, 128, 0)
    _, table = index_table(dev, 1, split, seed=0, identity=True)
    _, offsets = offsets_of((n,), dev)
    h = filled_h(dev, n, K)
    mixedgemm.moe_activate_quantize(t_from_bits(a_bits, dev), t_from_bits(b_bits, dev), offsets, table, h_out=h)
    torch.cuda.synchronize()
    got, want = bits_from_t(h), ma.h_oracle(a_bits, b_bits)
    ulp = o.bf16_ulp_distance(got, want)
    print(f"every finite bf16: {int((ulp != 0).sum())} values differ, at most {int(ulp.max())} bf16 ulp")
    worst = np.argmax(ulp)
    assert ulp.max() <= 1, f"silu({o.bf16_to_f32(a_bits.reshape(-1)[worst:worst + 1])[0]}) is {int(ulp.max())} bf16 ulps off"
    assert ((got & 0x7FFF) == 0)[(want & 0x7FFF) == 0].all(), "nonzero where the oracle is zero"


def test_non_finite_inputs_stay_in_their_rows(dev):
    import torch
    K, split, counts = 384, (128, 128, 128), (4, 0, 9, 3)
    E, n = len(counts), sum(counts)
    off, offsets = offsets_of(counts, dev)
    _, table = index_table(dev, E, split, seed=120)
    a_bits, b_bits, a, b = ab_on(dev, n, K, seed=121)
    h = filled_h(dev, n, K)
    clean = [u8(t) for t in mixedgemm.moe_activate_quantize(a, b, offsets, table, out=filled(dev, n, E, split), h_out=h)]
    clean_h = bits_from_t(h)
    bad_rows = [1, 5, 6, 15]
    pa, pb = a_bits.copy(), b_bits.copy()
    pa[1, [0, 77]] = [0x7F80, 0xFF80]                         # +inf, -inf in a
    pa[5, 300] = 0x7FC0                                       # NaN in a
    pb[6, [3, 200]] = [0xFF80, 0x7FC1]                        # -inf, NaN in b
    pb[15, 383] = 0x7F80
    h2 = filled_h(dev, n, K)
    dirty = [u8(t) for t in mixedgemm.moe_activate_quantize(t_from_bits(pa, dev), t_from_bits(pb, dev), offsets, table,
                                                            out=filled(dev, n, E, split), h_out=h2)]          # raises unless MM_OK
    torch.cuda.synchronize()
    keep = np.setdiff1d(np.arange(n), bad_rows)
    assert np.array_equal(bits_from_t(h2)[keep], clean_h[keep])
    for i, kseg in enumerate(split):
        assert np.array_equal(dirty[i][keep], clean[i][keep]), f"packed segment {i}"
        for e in range(E):
            M = off[e + 1] - off[e]
            if M == 0:
                continue
            rows = np.array([r - off[e] for r in keep if off[e] <= r < off[e + 1]])
            at = o.sf_offset(rows[:, None], np.arange(kseg // 32)[None, :], kseg)
            assert np.array_equal(sf_run(dirty[3 + i], off, e, kseg)[at], sf_run(clean[3 + i], off, e, kseg)[at]), f"scales of segment {i}"


# ---- 5. the block ---------------------------------------------------------------------------------------------------------------------
PACKED = ("BN", "BS", "BO", "SFBN", "SFBS", "SFBO")


class Built:
    """one configuration of tests/moe_block_oracle.py on the device: QLinearLayer triples and the three device tables"""

    def __init__(self, cfg_id, dev):
        import torch
        from micromix_amd.qlinear import QLinearLayer
        self.cfg = cfg = mb.CONFIGS[cfg_id]
        drawn = mb.draw_experts(cfg, dev, seed=1000 * (1 + "ABCDE".index(cfg_id)))

        def layer(w, bias, index, split):
            lin = torch.nn.Linear(w.size(1), w.size(0), bias=bias is not None, dtype=torch.bfloat16, device=dev)
            lin.weight.data = w
            if bias is not None:
                lin.bias.data = bias
            return QLinearLayer(lin, p8_num=split[2], p6_num=split[1], reorder_index=index, weight_mode=cfg["wmode"], rounding=cfg["rounding"])

        self.layers = [(layer(d["w"][0], d["bias"][0], d["idx1"], cfg["split1"]), layer(d["w"][1], d["bias"][1], d["idx1"], cfg["split1"]),
                        layer(d["w"][2], d["bias"][2], d["idx2"], cfg["split2"])) for d in drawn]
        split = (cfg["split1"], cfg["split1"], cfg["split2"])
        idx = [[t[i].reorder_index for t in self.layers] for i in range(3)]
        B = [[tuple(getattr(t[i], n) for n in PACKED) for t in self.layers] for i in range(3)]
        bias = [[t[i].bias for t in self.layers] for i in range(3)]
        self.tables = [mixedgemm.moe_expert_table(idx[i], B[i], *split[i], biases=bias[i]) for i in range(3)]


def launches(monkeypatch, block, x):
    """what one forward does, counted from Python: the mm_* entries it calls (queries aside) and the torch operators it dispatches"""
    import torch
    from torch.utils._python_dispatch import TorchDispatchMode
    calls, ops = [], []
    real = _lib.load()

    class Counting:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if not name.startswith("mm_"):
                return fn

            def counted(*a):
                calls.append(name)
                return fn(*a)
            return counted

    class Ops(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            ops.append(str(func))
            return func(*args, **(kwargs or {}))

    monkeypatch.setattr(_lib, "_lib", Counting())
    try:
        with Ops():
            block(x)
        torch.cuda.synchronize()
    finally:
        monkeypatch.undo()
    return [c for c in calls if not c.endswith("_supported")], [op for op in ops if op.startswith(("aten.silu", "aten.mul"))]


@pytest.fixture(scope="module")
def built(dev):
    cache = {}

    def get(cfg_id):
        if cfg_id not in cache:
            cache[cfg_id] = Built(cfg_id, dev)
        return cache[cfg_id]
    return get


def blocks(Bt, gate_w):
    from micromix_amd import SparseMoEBlock
    k = Bt.cfg["k"]
    return SparseMoEBlock(gate_w, Bt.layers, k), SparseMoEBlock(gate_w, Bt.layers, k, capturable=True), \
        SparseMoEBlock(gate_w, Bt.layers, k, capturable=True, fused_activation=True)


def chain(Bt, gate_w, x):
    """the fused block composed from the public ops, with h_out in the middle; returns (out, h)"""
    import torch
    cfg = Bt.cfg
    T = x.size(0)
    t1, t3, t2 = Bt.tables
    logits = torch.nn.functional.linear(x, gate_w)
    ids, w = mixedgemm.moe_route(logits, cfg["k"])
    offsets, sorted_token, slot_of = mixedgemm.moe_plan(ids, cfg["E"])
    q1 = mixedgemm.moe_quantize(x, sorted_token, offsets, t1)
    a = mixedgemm.moe_matmul(q1, offsets, t1, T, rounding=cfg["rounding"])
    b = mixedgemm.moe_matmul(q1, offsets, t3, T, rounding=cfg["rounding"])
    h = torch.zeros_like(a)
    q2 = mixedgemm.moe_activate_quantize(a, b, offsets, t2, h_out=h)
    y = mixedgemm.moe_matmul(q2, offsets, t2, T, rounding=cfg["rounding"])
    return mixedgemm.moe_combine(y, ids, w, slot_of), h


def assert_fused_block_is_the_chain(Bt, gate_w, x, label):
    import torch
    T, H = x.shape
    plain, _, fused = blocks(Bt, gate_w)
    want, h = chain(Bt, gate_w, x)
    _, want_logits = plain(x)
    lead = (2, T // 2) if T % 2 == 0 else (1, T)
    got, logits = fused(x)
    got3, logits3 = fused(x.reshape(*lead, H))
    got2, _ = fused(x)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want).all()) and float(want.float().abs().max()) > 0 and float(h.float().abs().max()) > 0
    assert torch.equal(logits, want_logits) and torch.equal(logits3, want_logits)
    assert torch.equal(got, want), f"{label}: the fused block differs from the chain of public ops"
    assert tuple(got3.shape) == (*lead, H) and torch.equal(got3.reshape(T, H), want) and torch.equal(got2, want), label


@pytest.mark.parametrize("T", [1, 7, 64, 65, 300])
def test_fused_block_a_is_the_chain_of_public_ops(dev, built, T):
    Bt = built("A")
    cfg = Bt.cfg
    gate = t_from_bits(o.f32_to_bf16((0.05 * np.random.default_rng(T).standard_normal((cfg["E"], cfg["H"]))).astype(np.float32)), dev)
    assert_fused_block_is_the_chain(Bt, gate, gen_bf16(dev, T, cfg["H"], 730 + T, "x"), f"A T={T}")


@pytest.mark.parametrize("name", ["A mixed", "B two launches", "C one token"])
def test_fused_block_with_scripted_routing(dev, built, name):
    cfg_id, T, counts = mb.SCRIPTED[name]
    Bt = built(cfg_id)
    cfg = Bt.cfg
    x_bits, _ = mb.scripted_x(counts, T, cfg["k"], bits_from_t(gen_bf16(dev, T, cfg["H"], 900 + T, "x")))
    assert_fused_block_is_the_chain(Bt, t_from_bits(mb.gate_unit_bits(cfg["E"], cfg["H"]), dev), t_from_bits(x_bits, dev), name)


def test_fused_activation_needs_capturable(dev, built):
    from micromix_amd import SparseMoEBlock
    Bt = built("A")
    gate = t_from_bits(mb.gate_unit_bits(Bt.cfg["E"], Bt.cfg["H"]), dev)
    with pytest.raises(ValueError, match="capturable"):
        SparseMoEBlock(gate, Bt.layers, Bt.cfg["k"], fused_activation=True)
    with pytest.raises(ValueError, match="capturable"):
        SparseMoEBlock(gate, Bt.layers, Bt.cfg["k"], capturable=False, fused_activation=True)


def test_one_launch_where_there_were_three_whatever_e_is(dev, built, monkeypatch):
    """The fused block calls the library as often as the capturable one -- eight times at E = 8 and at E = 64, with
    mm_moe_activate_quantize in the place of the second mm_moe_quantize -- and dispatches neither of the two torch operators (silu,
    mul) that the capturable block runs in front of that quantizer: ten launches become eight."""
    want = ["mm_moe_route", "mm_moe_plan", "mm_moe_quantize", "mm_moe_matmul", "mm_moe_matmul", "mm_moe_activate_quantize", "mm_moe_matmul", "mm_moe_combine"]
    seen = {}
    for cfg_id, name in (("A", "A largest 16"), ("C", "C one token")):
        _, T, counts = mb.SCRIPTED[name]
        Bt = built(cfg_id)
        cfg = Bt.cfg
        x_bits, _ = mb.scripted_x(counts, T, cfg["k"], bits_from_t(gen_bf16(dev, T, cfg["H"], 900 + T, "x")))
        _, capt, fused = blocks(Bt, t_from_bits(mb.gate_unit_bits(cfg["E"], cfg["H"]), dev))
        x = t_from_bits(x_bits, dev)
        fused(x), capt(x)
        seen[cfg_id] = (launches(monkeypatch, fused, x), launches(monkeypatch, capt, x))
    for cfg_id in "AC":
        (calls, ops), (capt_calls, capt_ops) = seen[cfg_id]
        assert calls == want and ops == [], seen
        assert len(capt_calls) == 8 and len(capt_ops) == 2 and capt_calls == [c.replace("activate_", "") for c in want], seen
        assert len(calls) + len(ops) == len(capt_calls) + len(capt_ops) - 2


# T = 16 on block A (E 8, k 2): the captured routing first, then other experts empty and the largest group across 16 / 17
ROUTINGS_16 = [(4,) * 8, (16, 16, 0, 0, 0, 0, 0, 0), (0, 1, 0, 15, 0, 0, 16, 0), (0, 0, 9, 0, 7, 0, 0, 16)]


def test_one_capture_of_the_fused_block_replays_on_other_routings(dev, built):
    import torch
    T = 16
    Bt = built("A")
    cfg = Bt.cfg
    E, k, H = cfg["E"], cfg["k"], cfg["H"]
    gate = t_from_bits(mb.gate_unit_bits(E, H), dev)
    _, _, fused = blocks(Bt, gate)
    inputs = []
    for i, counts in enumerate(ROUTINGS_16):
        bits, _ = mb.scripted_x(counts, T, k, bits_from_t(gen_bf16(dev, T, H, 750 + 10 * T + i, "x")))
        inputs.append((counts, t_from_bits(bits, dev)))
    static_in = inputs[0][1].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                             # warm-up outside the capture, as micromix_amd/graph.py does
        for _ in range(2):
            fused(static_in)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                             # a read of device data on the host would end the capture with an error
        static_out, static_logits = fused(static_in)
    for counts, x in inputs + inputs[:1]:                     # ... and back to the captured routing
        static_in.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        got, got_logits = static_out.clone(), static_logits.clone()
        want, want_logits = fused(x)
        torch.cuda.synchronize()
        assert np.array_equal(np.bincount(u8(mixedgemm.moe_route(want_logits, k)[0]).reshape(-1), minlength=E), counts), "the routing is not the scripted one"
        assert torch.equal(got_logits, want_logits)
        assert bool(torch.isfinite(want).all()) and float(want.float().abs().max()) > 0
        assert torch.equal(got, want), f"rows per expert {counts}: the replay differs from the eager fused block"
