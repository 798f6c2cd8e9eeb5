"""GPU tests of mixedgemm.moe_gate_up_activate and of SparseMoEBlock(capturable=True, fused_gate_up=...):

  1. exact: for every slot an expert owns, the packed rows (whole) and the scale bytes at sf_offset are byte for byte
     moe_activate_quantize(a, b, offsets, w2's table) with a, b the rows the tiled kernels without split-K give the expert for w1 and
     w3 -- moe_matmul's own output above 64 rows, matmul_grouped on the expert's rows padded with zero rows to 65 below -- with all
     three output formats, eight slabs of K, experts of 0 / 1 / 64 / 65 / 127 / 128 / 129 / 257 rows, empty experts at the front /
     middle / end, all rows in one expert, E = 64 with n = 8, an identity w2 index, both rounding modes;
  2. untouched: outputs pre-filled with 0xFF keep the packed rows from offsets[E] on, the scale tiles outside every run, everything
     after junk offsets, and the rows of an expert above max_rows;
  3. the 256-row tile kernel (n = 3 400, I = 1 024: the bound of 272 workgroups exceeds one round), asserted through the describe string;
  4. bounds: every operand at the end of an allocation of its own (tests/moe_gate_up_bounds_probe.py, a child process);
  5. the block: bit-equal to the chain of public ops; bit-equal to fused_activation=True where every expert with rows has more than
     64; two launches fewer, whatever E; one capture at T = 16 replayed on other routings; an integer threshold switches paths.
No time is measured here."""
import os
import subprocess
import sys

import numpy as np
import pytest

import moe_block_oracle as mb
import test_moe_activate_gpu as act
from conftest import bits_from_t, t_from_bits, u8
from micromix_amd import _lib, mixedgemm
from model_case import gen_bf16, gen_index
from oracle import mx_oracle as o

pytestmark = pytest.mark.gpu


class Experts:
    """E experts' fp4 w1 / w3 [I, H] with reorder indices of their own, the three tables the reference chain reads (w1, w3, and w2's
    index with zero weights) and the packed w1 | w3 table under test; built once per configuration"""

    def __init__(self, dev, E, H, split1, I, split2, seed, identity2=False):
        import torch
        self.E, self.H, self.I, self.split1, self.split2 = E, H, I, split1, split2
        self.idx1 = [gen_index(dev, H, seed + 3 * e) for e in range(E)]
        self.idx2 = [torch.arange(I, dtype=torch.int16, device=dev) if identity2 else gen_index(dev, I, seed + 3 * e + 1) for e in range(E)]
        self.w1 = [mixedgemm.reorder_quantize_w4(gen_bf16(dev, I, H, seed + 7 * e, "w") * 4, self.idx1[e], *split1) for e in range(E)]
        self.w3 = [mixedgemm.reorder_quantize_w4(gen_bf16(dev, I, H, seed + 7 * e + 1, "w") * 4, self.idx1[e], *split1) for e in range(E)]
        self.t1 = mixedgemm.moe_expert_table(self.idx1, self.w1, *split1)
        self.t3 = mixedgemm.moe_expert_table(self.idx1, self.w3, *split1)
        z = lambda *s: torch.zeros(s, dtype=torch.uint8, device=dev)
        B2 = (z(16, split2[0] // 2), z(16, split2[1] // 2), z(16, split2[2] // 2), z(128 * split2[0] // 32), z(128 * split2[1] // 32), z(128 * split2[2] // 32))
        self.t2 = mixedgemm.moe_expert_table(self.idx2, [B2] * E, *split2)
        self.gu = mixedgemm.moe_gate_up_table(self.idx1, self.w1, self.w3, self.idx2, split1, split2)
        assert self.gu.N == 2 * I and not self.gu.has_bias and self.gu.wmode == _lib.MM_W_FP4


CONFIGS = {
    "three formats": dict(E=8, H=384, split1=(128, 128, 128), I=384, split2=(128, 128, 128), seed=100),
    "eight slabs": dict(E=8, H=1024, split1=(512, 128, 384), I=256, split2=(128, 0, 128), seed=200),
    "identity idx2": dict(E=8, H=384, split1=(128, 128, 128), I=384, split2=(128, 128, 128), seed=300, identity2=True),
    "E 64": dict(E=64, H=384, split1=(128, 128, 128), I=384, split2=(128, 128, 128), seed=400),
    "wide": dict(E=8, H=384, split1=(128, 128, 128), I=1024, split2=(512, 256, 256), seed=500),
}


@pytest.fixture(scope="module")
def experts(dev):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Experts(dev, **CONFIGS[name])
        return cache[name]
    return get


def reference_ab(X, x, off, offsets, q1, max_rows, rounding):
    """a, b bf16 [n, I]: moe_matmul's rows, and for every expert of 1 .. 64 rows the rows the tiled kernels give it -- matmul_grouped on
    its bf16 rows padded with zero rows to 65 (rows are independent, and the grouped tiled launch never splits K)"""
    import torch
    n = x.size(0)
    small = [e for e in range(X.E) if 1 <= off[e + 1] - off[e] <= min(64, max_rows)]
    pad = []
    for e in small:
        p = torch.zeros((65, X.H), dtype=torch.bfloat16, device=x.device)
        p[: off[e + 1] - off[e]] = x[off[e]:off[e + 1]]
        pad.append(p)
    qs = mixedgemm.reorder_quantize_x_grouped(pad, [X.idx1[e] for e in small], *X.split1) if small else []
    res = []
    for table, W in ((X.t1, X.w1), (X.t3, X.w3)):
        d = torch.full((n, X.I), -1, dtype=torch.int16, device=x.device).view(torch.bfloat16)
        mixedgemm.moe_matmul(q1, offsets, table, max_rows, rounding=rounding, out=d)
        if small:
            outs = mixedgemm.matmul_grouped(qs, [W[e] for e in small], rounding=rounding)
            for e, t in zip(small, outs):
                d[off[e]:off[e + 1]] = t[: off[e + 1] - off[e]]
        res.append(d)
    return res


def run_case(dev, X, counts, rounding="reference", max_rows=None, extra=0, seed=1):
    """counts: rows per expert; extra: slots behind offsets[E] that nobody owns.  Asserts section 4 of the contract and returns the
    describe string of the launch"""
    import torch
    owned, n = sum(counts), sum(counts) + extra
    max_rows = max(counts) if max_rows is None else max_rows
    off, offsets = act.offsets_of(counts, dev)
    x = gen_bf16(dev, n, X.H, seed, "x")
    q1 = mixedgemm.moe_quantize(x, None, offsets, X.t1, n=n, out=tuple(torch.zeros_like(t) for t in act.filled(dev, n, X.E, X.split1)))
    a, b = reference_ab(X, x, off, offsets, q1, max_rows, rounding)
    want = [u8(t) for t in mixedgemm.moe_activate_quantize(a, b, offsets, X.t2, out=act.filled(dev, n, X.E, X.split2))]
    assert mixedgemm.moe_gate_up_activate_supported(max_rows, X.gu, X.split2)
    got = [u8(t) for t in mixedgemm.moe_gate_up_activate(q1, offsets, X.gu, max_rows, X.split2, rounding=rounding, out=act.filled(dev, n, X.E, X.split2))]
    torch.cuda.synchronize()
    live = [e for e in range(X.E) if 1 <= counts[e] <= max_rows]
    assert live and any((want[i][off[e]:off[e + 1]] != 0xFF).any() for e in live for i in range(3) if X.split2[i])
    for i, kseg in enumerate(X.split2):
        if kseg == 0:
            continue
        for e in range(X.E):
            rows = slice(off[e], off[e + 1])
            if e in live:
                bad = np.nonzero((got[i][rows] != want[i][rows]).any(axis=1))[0]
                assert bad.size == 0, f"segment {i}, expert {e} ({counts[e]} rows): packed rows {bad[:8]} differ"
            else:
                assert (got[i][rows] == 0xFF).all(), f"segment {i}: packed rows of skipped expert {e} were written"
        assert (got[i][owned:] == 0xFF).all(), f"segment {i}: packed rows from offsets[E] on were written"
        outside = np.ones(got[3 + i].shape, dtype=bool)
        for e in live:
            run_got, run_want = act.sf_run(got[3 + i], off, e, kseg), act.sf_run(want[3 + i], off, e, kseg)
            at = o.sf_valid_offsets(counts[e], kseg)
            bad = np.nonzero(run_got[at] != run_want[at])[0]
            assert bad.size == 0, f"segment {i}, expert {e} ({counts[e]} rows): {bad.size} scale bytes of owned rows differ"
            act.sf_run(outside, off, e, kseg)[:] = False
        assert (got[3 + i][outside] == 0xFF).all(), f"segment {i}: a scale tile outside every expert's run was written"
    return mixedgemm.moe_gate_up_activate_describe(X.gu, n)


ROWS = {
    "0 1 64 65 127 128 129 257": (0, 1, 64, 65, 127, 128, 129, 257),
    "empty front middle end": (0, 5, 0, 0, 70, 3, 0, 0),
    "all in one expert": (0, 0, 0, 200, 0, 0, 0, 0),
}


@pytest.mark.parametrize("rounding", ["reference", "fused"])
@pytest.mark.parametrize("rows", list(ROWS))
def test_three_formats_byte_for_byte(dev, experts, rows, rounding):
    what = run_case(dev, experts("three formats"), ROWS[rows], rounding, extra=6, seed=len(rows))
    assert "g128" in what, what


@pytest.mark.parametrize("rounding", ["reference", "fused"])
def test_eight_slabs_byte_for_byte(dev, experts, rounding):
    run_case(dev, experts("eight slabs"), (3, 0, 130, 66, 0, 64, 9, 0), rounding, seed=21)


def test_identity_w2_index_byte_for_byte(dev, experts):
    """no permutation of the weight rows: an epilogue bug would show here too, a permutation bug only in the other cases"""
    run_case(dev, experts("identity idx2"), (0, 1, 64, 65, 127, 128, 129, 30), seed=22)


def test_e_64_with_8_rows(dev, experts):
    run_case(dev, experts("E 64"), tuple(1 if e in (3, 9, 17, 26, 31, 40, 57, 63) else 0 for e in range(64)), seed=23)


def test_an_expert_above_max_rows_is_skipped_whole(dev, experts):
    run_case(dev, experts("three formats"), (0, 5, 129, 0, 100, 3, 0, 101), max_rows=100, extra=3, seed=24)


def test_junk_offsets_write_nothing(dev, experts):
    import torch
    X = experts("three formats")
    n = 40
    _, offsets = act.offsets_of((5, 5, 5, 5, 5, 5, 5, 5), dev)
    q1 = mixedgemm.moe_quantize(gen_bf16(dev, n, X.H, 25, "x"), None, offsets, X.t1)
    for junk in ([5, 3] + [n + 9] * (X.E - 1), [-4] * (X.E + 1), [n + 1] * (X.E + 1), [0, -3] + [n] * (X.E - 1)):
        out = mixedgemm.moe_gate_up_activate(q1, torch.tensor(junk, dtype=torch.int32, device=dev), X.gu, n, X.split2, out=act.filled(dev, n, X.E, X.split2))
        torch.cuda.synchronize()
        assert all((u8(t) == 0xFF).all() for t in out), junk


def test_the_256_row_tile_kernel(dev, experts):
    """n = 3 400, E = 8, I = 1 024: (3400 / 128 + 8) * 8 = 272 workgroups of 128-row tiles exceed the 256 CUs, so the launch takes the
    256-row tiles; one expert across 256 / 257 rows"""
    lib = _lib.load()
    X = experts("wide")
    counts = (256, 257, 1, 64, 600, 0, 1000, 1222)
    assert sum(counts) == 3400
    import torch
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    what = run_case(dev, X, counts, seed=26)
    assert ("g256" in what and "256x256" in what) == ((3400 // 128 + 8) * 8 > cus), (what, cus)
    assert cus != 256 or what.startswith("mm::g256::mx_gemm256_moe_act_kernel x 168 workgroups"), what
    assert lib.mm_moe_gate_up_activate_describe(8, 771, 384).decode().startswith("mm::g128::mx_gemm256_moe_act_kernel x 42 workgroups") or cus < 42


def test_gate_up_activate_stays_inside_its_operands():
    """tests/moe_gate_up_bounds_probe.py in a child process (a memory fault would kill it, not this run)"""
    probe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "moe_gate_up_bounds_probe.py")
    r = subprocess.run([sys.executable, probe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"the probe died (exit {r.returncode}):\n{r.stdout}\n{r.stderr[-2000:]}"
    lines = [l.split() for l in r.stdout.splitlines() if l.startswith("case")]
    assert len(lines) == 4 and "done" in r.stdout, r.stdout
    for _, label, got, want in lines:
        assert got == want, f"{label}: other bytes with the operands at the end of their allocations"


# ---- 5. the block ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built(dev):
    cache = {}

    def get(cfg_id):
        if cfg_id not in cache:
            Bt = act.Built(cfg_id, dev)
            cfg = Bt.cfg
            idx1, idx2 = [t[0].reorder_index for t in Bt.layers], [t[2].reorder_index for t in Bt.layers]
            B = [[tuple(getattr(t[i], n) for n in act.PACKED) for t in Bt.layers] for i in range(2)]
            Bt.gu = mixedgemm.moe_gate_up_table(idx1, B[0], B[1], idx2, cfg["split1"], cfg["split2"])
            cache[cfg_id] = Bt
        return cache[cfg_id]
    return get


def gate_up_block(Bt, gate_w, flag=True):
    from micromix_amd import SparseMoEBlock
    return SparseMoEBlock(gate_w, Bt.layers, Bt.cfg["k"], capturable=True, fused_gate_up=flag)


def chain(Bt, gate_w, x):
    """the block composed from the public ops: route, plan, moe_quantize, moe_gate_up_activate, moe_matmul, combine"""
    import torch
    cfg = Bt.cfg
    T = x.size(0)
    t1, _, t2 = Bt.tables
    ids, w = mixedgemm.moe_route(torch.nn.functional.linear(x, gate_w), cfg["k"])
    offsets, sorted_token, slot_of = mixedgemm.moe_plan(ids, cfg["E"])
    q1 = mixedgemm.moe_quantize(x, sorted_token, offsets, t1)
    q2 = mixedgemm.moe_gate_up_activate(q1, offsets, Bt.gu, T, cfg["split2"], rounding=cfg["rounding"])
    y = mixedgemm.moe_matmul(q2, offsets, t2, T, rounding=cfg["rounding"])
    return mixedgemm.moe_combine(y, ids, w, slot_of)


def assert_block_is_the_chain(Bt, gate_w, x, label):
    import torch
    T, H = x.shape
    block = gate_up_block(Bt, gate_w)
    want = chain(Bt, gate_w, x)
    lead = (2, T // 2) if T % 2 == 0 else (1, T)
    got, logits = block(x)
    got3, logits3 = block(x.reshape(*lead, H))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want).all()) and float(want.float().abs().max()) > 0
    assert torch.equal(logits, torch.nn.functional.linear(x, gate_w)) and torch.equal(logits3, logits)
    assert torch.equal(got, want), f"{label}: the block differs from the chain of public ops"
    assert tuple(got3.shape) == (*lead, H) and torch.equal(got3.reshape(T, H), want), label


@pytest.mark.parametrize("T", [1, 7, 65, 300])
def test_block_is_the_chain_of_public_ops(dev, built, T):
    Bt = built("A")
    cfg = Bt.cfg
    gate = t_from_bits(o.f32_to_bf16((0.05 * np.random.default_rng(T).standard_normal((cfg["E"], cfg["H"]))).astype(np.float32)), dev)
    assert_block_is_the_chain(Bt, gate, gen_bf16(dev, T, cfg["H"], 830 + T, "x"), f"A T={T}")


def scripted(Bt, dev, T, counts, seed):
    cfg = Bt.cfg
    bits, _ = mb.scripted_x(counts, T, cfg["k"], bits_from_t(gen_bf16(dev, T, cfg["H"], seed, "x")))
    return t_from_bits(mb.gate_unit_bits(cfg["E"], cfg["H"]), dev), t_from_bits(bits, dev)


def test_block_with_scripted_routing(dev, built):
    _, T, counts = mb.SCRIPTED["A mixed"]
    Bt = built("A")
    gate, x = scripted(Bt, dev, T, counts, 901)
    assert_block_is_the_chain(Bt, gate, x, "A mixed")


def test_block_is_fused_activation_where_every_expert_has_more_than_64_rows(dev, built):
    import torch
    from micromix_amd import SparseMoEBlock
    Bt = built("A")
    T, counts = 200, (0, 0, 65, 70, 0, 135, 0, 130)
    gate, x = scripted(Bt, dev, T, counts, 902)
    want, want_logits = SparseMoEBlock(gate, Bt.layers, Bt.cfg["k"], capturable=True, fused_activation=True)(x)
    got, logits = gate_up_block(Bt, gate)(x)
    torch.cuda.synchronize()
    assert np.array_equal(np.bincount(u8(mixedgemm.moe_route(logits, Bt.cfg["k"])[0]).reshape(-1), minlength=Bt.cfg["E"]), counts)
    assert torch.equal(logits, want_logits) and float(want.float().abs().max()) > 0
    assert torch.equal(got, want), "fused_gate_up differs from fused_activation although every expert runs on the tiled kernels in both"


def test_construction_errors(dev, built):
    from micromix_amd import SparseMoEBlock
    Bt = built("A")
    gate = t_from_bits(mb.gate_unit_bits(Bt.cfg["E"], Bt.cfg["H"]), dev)
    for flag in (True, 32):
        with pytest.raises(ValueError, match="capturable"):
            SparseMoEBlock(gate, Bt.layers, Bt.cfg["k"], fused_gate_up=flag)
    Bw = act.Built("B", dev)                                  # "w"-mode weights, biases on odd experts
    with pytest.raises(ValueError):
        SparseMoEBlock(t_from_bits(mb.gate_unit_bits(Bw.cfg["E"], Bw.cfg["H"]), dev), Bw.layers, Bw.cfg["k"], capturable=True, fused_gate_up=True)


WANT_CALLS = ["mm_moe_route", "mm_moe_plan", "mm_moe_quantize", "mm_moe_gate_up_activate", "mm_moe_matmul", "mm_moe_combine"]


def test_two_launches_fewer_whatever_e_is(dev, built, monkeypatch):
    from micromix_amd import SparseMoEBlock
    for cfg_id, name in (("A", "A largest 16"), ("C", "C one token")):
        _, T, counts = mb.SCRIPTED[name]
        Bt = built(cfg_id)
        gate, x = scripted(Bt, dev, T, counts, 903)
        fused, old = gate_up_block(Bt, gate), SparseMoEBlock(gate, Bt.layers, Bt.cfg["k"], capturable=True, fused_activation=True)
        fused(x), old(x)
        calls, ops = act.launches(monkeypatch, fused, x)
        old_calls, old_ops = act.launches(monkeypatch, old, x)
        assert calls == WANT_CALLS and ops == [] and old_ops == [], (cfg_id, calls, ops)
        assert len(calls) == len(old_calls) - 2 == 6, (cfg_id, calls, old_calls)


def test_an_integer_threshold_switches_the_path(dev, built, monkeypatch):
    Bt = built("A")
    cfg = Bt.cfg
    gate = t_from_bits(mb.gate_unit_bits(cfg["E"], cfg["H"]), dev)
    block = gate_up_block(Bt, gate, 32)
    for T, new in ((16, False), (32, True), (33, True)):
        x = gen_bf16(dev, T, cfg["H"], 910 + T, "x")
        block(x)
        calls, ops = act.launches(monkeypatch, block, x)
        if new:
            assert calls == WANT_CALLS and ops == [], (T, calls)
        else:
            assert calls == ["mm_moe_route", "mm_moe_plan", "mm_moe_quantize", "mm_moe_matmul", "mm_moe_matmul", "mm_moe_quantize", "mm_moe_matmul", "mm_moe_combine"] \
                and len(ops) == 2, (T, calls, ops)


def test_one_capture_replays_on_other_routings(dev, built):
    import torch
    T = 16
    Bt = built("A")
    cfg = Bt.cfg
    E, k, H = cfg["E"], cfg["k"], cfg["H"]
    gate = t_from_bits(mb.gate_unit_bits(E, H), dev)
    block = gate_up_block(Bt, gate)
    inputs = []
    for i, counts in enumerate(act.ROUTINGS_16):
        bits, _ = mb.scripted_x(counts, T, k, bits_from_t(gen_bf16(dev, T, H, 950 + i, "x")))
        inputs.append((counts, t_from_bits(bits, dev)))
    static_in = inputs[0][1].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                             # warm-up outside the capture, as micromix_amd/graph.py does
        for _ in range(2):
            block(static_in)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                             # a read of device data on the host would end the capture with an error
        static_out, static_logits = block(static_in)
    for counts, x in inputs + inputs[:1]:
        static_in.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        got, got_logits = static_out.clone(), static_logits.clone()
        want, want_logits = block(x)
        torch.cuda.synchronize()
        assert np.array_equal(np.bincount(u8(mixedgemm.moe_route(want_logits, k)[0]).reshape(-1), minlength=E), counts), "the routing is not the scripted one"
        assert torch.equal(got_logits, want_logits)
        assert bool(torch.isfinite(want).all()) and float(want.float().abs().max()) > 0
        assert torch.equal(got, want), f"rows per expert {counts}: the replay differs from the eager block"
