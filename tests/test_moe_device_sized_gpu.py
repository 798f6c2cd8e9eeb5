"""GPU tests of the device-sized grouped launches and of SparseMoEBlock(capturable=True):

  1. mixedgemm.moe_quantize byte for byte reorder_quantize_x_grouped on the same rows -- packed rows as slices, scale bytes on the rows
     that exist at the run the rule assigns -- through row_of_slot = sorted_token and through NULL on gathered rows, both quantizer
     modes, every output pre-filled with 0xFF: what no expert owns is still 0xFF after calls whose ids and rows include bad values;
  2. mixedgemm.moe_matmul bit-equal to matmul_grouped(outs=), both roundings, w4 and "w", with and without biases, max_rows in T, 64,
     65, n: D pre-filled with NaN, every row of an expert within max_rows written, the rows of a larger expert still NaN;
  3. the capturable block bit-equal to the default block, 2-D and 3-D input, two calls;
  4. one capture of forward per T replayed on other routings (other experts empty, the largest group across the 16 / 32 / 48 / 64
     tier edges, groups across 64 / 65), each replay bit-equal to the eager default block on the same input;
  5. the number of calls into the library does not grow with E.

The blocks and the rows per expert are those of tests/moe_block_oracle.py (A: E 8, k 2, w4; B: E 16, k 4, "w", biases; C: E 64, k 8)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import moe_block_oracle as mb
from conftest import bits_from_t, t_from_bits, u8
from micromix_amd import _lib, mixedgemm
from model_case import gen_bf16
from oracle import mx_oracle as o

pytestmark = pytest.mark.gpu
PACKED = ("BN", "BS", "BO", "SFBN", "SFBS", "SFBO")
CASES = [n for n in mb.SCRIPTED if n[0] in "ABC"]


class Built:
    """one configuration on the device: QLinearLayer triples as tests/test_moe_block_gpu.py draws them, and the three device tables"""

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
        self.split = (cfg["split1"], cfg["split1"], cfg["split2"])
        self.idx = [[t[i].reorder_index for t in self.layers] for i in range(3)]
        self.B = [[tuple(getattr(t[i], n) for n in PACKED) for t in self.layers] for i in range(3)]
        self.bias = [[t[i].bias for t in self.layers] for i in range(3)]
        self.tables = [mixedgemm.moe_expert_table(self.idx[i], self.B[i], *self.split[i], biases=self.bias[i]) for i in range(3)]


@pytest.fixture(scope="module")
def built(dev):
    cache = {}

    def get(cfg_id):
        if cfg_id not in cache:
            cache[cfg_id] = Built(cfg_id, dev)
        return cache[cfg_id]
    return get


def planned(dev, name):
    """(Built-independent) the scripted plan of a case on the device: cfg, T, offsets (host list and device), sorted_token"""
    cfg_id, T, counts = mb.SCRIPTED[name]
    cfg = mb.CONFIGS[cfg_id]
    import torch
    ids = torch.from_numpy(mb.scripted_ids(counts, T, cfg["k"])).to(dev)
    offsets, sorted_token, _ = mixedgemm.moe_plan(ids, cfg["E"])
    off = offsets.tolist()
    assert np.array_equal(np.diff(off), counts)
    return cfg_id, cfg, T, off, offsets, sorted_token


def sf_run(sf, off, e, kseg):
    """expert e's run of a packed scale tensor, by the rule: tile off[e] // 128 + e, ceil(M / 128) tiles"""
    tile = 128 * kseg // 32
    return sf[(off[e] // 128 + e) * tile:][: (off[e + 1] - off[e] + 127) // 128 * tile]


def assert_packed_equals_grouped(got, want, off, split, E, n, label, w4=False, skip=()):
    """got: moe_quantize's 6-tuple (host arrays, pre-filled with 0xFF); want[e]: the expert's own 6-tuple.  Everything an expert owns is
    the expert's bytes; every other byte is still 0xFF.  skip: slots that the call must have left untouched."""
    for i, kseg in enumerate(split):
        if kseg == 0:
            continue
        packed = np.full_like(got[i], 0xFF)
        sf = np.full_like(got[3 + i], 0xFF)
        assert sf.size == (n // 128 + E) * 128 * kseg // 32
        for e in range(E):
            M = off[e + 1] - off[e]
            if M == 0:
                continue
            packed[off[e]:off[e + 1]] = want[e][i]
            valid = o.sf_valid_offsets(M, kseg)
            sf_run(sf, off, e, kseg)[valid] = want[e][3 + i][valid]
        for s in skip:
            e = int(np.searchsorted(off, s, side="right")) - 1
            packed[s] = 0xFF
            sf_run(sf, off, e, kseg)[o.sf_valid_offsets(off[e + 1] - off[e], kseg).reshape(off[e + 1] - off[e], -1)[s - off[e]]] = 0xFF
        assert np.array_equal(got[i], packed), f"{label}: packed segment {i}"
        assert np.array_equal(got[3 + i], sf), f"{label}: scale bytes of segment {i} (or a byte that no expert owns was written)"


def filled_outputs(dev, n, E, split, w4):
    import torch
    widths = (split[0] // 2, split[1] // 2 if w4 else split[1] // 4 * 3, split[2] // 2 if w4 else split[2])
    return tuple(torch.full((n, w), 0xFF, dtype=torch.uint8, device=dev) for w in widths) + \
        tuple(torch.full((mixedgemm.moe_sf_bytes(n, E, k),), 0xFF, dtype=torch.uint8, device=dev) for k in split)


# ---- 1. the quantizer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("mode", ["x", "w4"])
def test_moe_quantize_is_the_grouped_quantizer_byte_for_byte(dev, built, name, mode):
    cfg_id, cfg, T, off, offsets, sorted_token = planned(dev, name)
    Bt = built(cfg_id)
    E, k, H = cfg["E"], cfg["k"], cfg["H"]
    n, split, w4 = T * k, cfg["split1"], mode == "w4"
    x = gen_bf16(dev, T, H, 700 + T, "x")
    xs = mixedgemm.moe_gather(x, sorted_token)
    rows = [xs[off[e]:off[e + 1]] for e in range(E)]
    if w4:
        want = [mixedgemm.reorder_quantize_w4(r, i, *split) if r.size(0) else None for r, i in zip(rows, Bt.idx[0])]
    else:
        want = mixedgemm.reorder_quantize_x_grouped(rows, Bt.idx[0], *split)
    want = [[u8(t) for t in w] if w is not None else None for w in want]
    got_a = mixedgemm.moe_quantize(x, sorted_token, offsets, Bt.tables[0], mode=mode, out=filled_outputs(dev, n, E, split, w4))
    got_b = mixedgemm.moe_quantize(xs, None, offsets, Bt.tables[0], mode=mode, out=filled_outputs(dev, n, E, split, w4))
    assert_packed_equals_grouped([u8(t) for t in got_a], want, off, split, E, n, f"{name} {mode} through sorted_token", w4)
    assert_packed_equals_grouped([u8(t) for t in got_b], want, off, split, E, n, f"{name} {mode} on gathered rows", w4)


@pytest.mark.parametrize("name", ["A mixed", "C one token"])
def test_moe_quantize_leaves_what_no_expert_owns(dev, built, name):
    """ids outside [0, E) upstream: the plan counts fewer pairs, so the slots from offsets[E] on belong to nobody and hold
    sorted_token = -1; and row indices outside [0, T) in owned slots.  Those slots' packed rows and scale bytes stay 0xFF."""
    import torch
    cfg_id, T, counts = mb.SCRIPTED[name]
    cfg = mb.CONFIGS[cfg_id]
    Bt = built(cfg_id)
    E, k, H, split = cfg["E"], cfg["k"], cfg["H"], cfg["split1"]
    n = T * k
    ids = mb.scripted_ids(counts, T, k).copy()
    flat = ids.reshape(-1)
    flat[[0, n // 2, n - 1][: min(3, n - 1)]] = [-1, E, 77][: min(3, n - 1)]
    offsets, sorted_token, _ = mixedgemm.moe_plan(torch.from_numpy(ids).to(dev), E)
    off = offsets.tolist()
    assert off[E] == n - min(3, n - 1) and (u8(sorted_token)[off[E]:] == -1).all()
    bad = sorted_token.clone()
    skip = sorted({0, off[E] // 2, off[E] - 1})
    bad[torch.tensor(skip, device=dev)] = torch.tensor([-5, T, 2 ** 30][: len(skip)], dtype=torch.int32, device=dev)
    x = gen_bf16(dev, T, H, 710 + T, "x")
    xs = mixedgemm.moe_gather(x, sorted_token)
    want = [[u8(t) for t in w] for w in mixedgemm.reorder_quantize_x_grouped([xs[off[e]:off[e + 1]] for e in range(E)], Bt.idx[0], *split)]
    got = mixedgemm.moe_quantize(x, bad, offsets, Bt.tables[0], out=filled_outputs(dev, n, E, split, False))
    assert_packed_equals_grouped([u8(t) for t in got], want, off, split, E, n, name, skip=skip)
    # offsets that are no plan's: decreasing, negative, past n -- nothing may be written at all
    for junk in ([5, 3] + [n + 9] * (E - 1), [-4] * (E + 1), [n + 1] * (E + 1)):
        out = mixedgemm.moe_quantize(x, sorted_token, torch.tensor(junk, dtype=torch.int32, device=dev), Bt.tables[0],
                                     out=filled_outputs(dev, n, E, split, False))
        torch.cuda.synchronize()
        assert all((u8(t) == 0xFF).all() for t in out), junk


# ---- 2. the GEMM --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_moe_matmul_is_matmul_grouped_bit_for_bit(dev, built, name):
    import torch
    cfg_id, cfg, T, off, offsets, sorted_token = planned(dev, name)
    Bt = built(cfg_id)
    E, k = cfg["E"], cfg["k"]
    n = T * k
    counts = np.diff(off)
    for layer in (0, 2):                                      # w1 over H, w2 over I (C: the layer with the biases)
        split, K = Bt.split[layer], sum(Bt.split[layer])
        N = Bt.B[layer][0][0].size(0)
        rows = gen_bf16(dev, n, K, 720 + T + layer, "x")
        q = mixedgemm.moe_quantize(rows, None, offsets, Bt.tables[layer])
        qe = mixedgemm.reorder_quantize_x_grouped([rows[off[e]:off[e + 1]] for e in range(E)], Bt.idx[layer], *split)
        for rounding in ("reference", "fused"):
            want = torch.zeros((n, N), dtype=torch.bfloat16, device=dev)
            mixedgemm.matmul_grouped(qe, Bt.B[layer], biases=Bt.bias[layer] if any(b is not None for b in Bt.bias[layer]) else None,
                                     rounding=rounding, outs=[want[off[e]:off[e + 1]] for e in range(E)])
            want_bits = bits_from_t(want)
            for max_rows in sorted({T, 64, 65, n}):
                D = torch.full((n, N), float("nan"), dtype=torch.bfloat16, device=dev)
                got = mixedgemm.moe_matmul(q, offsets, Bt.tables[layer], max_rows, rounding=rounding, out=D)
                assert got is D
                got_bits = bits_from_t(D)
                label = f"{name} layer {layer} {rounding} max_rows {max_rows}"
                for e in range(E):
                    own = got_bits[off[e]:off[e + 1]]
                    if counts[e] > max_rows:                  # the caller's bound was wrong for this expert: skipped whole
                        assert np.isnan(o.bf16_to_f32(own)).all(), f"{label}: expert {e} ({counts[e]} rows) was not skipped whole"
                    else:
                        assert not np.isnan(o.bf16_to_f32(own)).any(), f"{label}: expert {e} ({counts[e]} rows) has unwritten rows"
                        assert np.array_equal(own, want_bits[off[e]:off[e + 1]]), f"{label}: expert {e} ({counts[e]} rows) differs"
    assert any(c > 64 for c in counts) or name != "A mixed"


def test_moe_matmul_without_a_segment_writes_zeros_to_owned_rows(dev, built):
    import torch
    cfg_id, cfg, T, off, offsets, _ = planned(dev, "A largest 16")
    Bt, n = built(cfg_id), T * cfg["k"]
    lib = _lib.load()
    D = torch.full((n + 4, 256), float("nan"), dtype=torch.bfloat16, device=dev)
    st = lib.mm_moe_matmul(None, None, None, None, None, None, offsets.data_ptr(), Bt.tables[0].tensor.data_ptr(), cfg["E"], n + 4, T, 256, 0, 0, 0,
                           _lib.MM_W_FP4, 0, D.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert st == _lib.MM_OK
    bits = bits_from_t(D)
    assert (bits[:n] == 0).all() and np.isnan(o.bf16_to_f32(bits[n:])).all()


# ---- 3. the block -------------------------------------------------------------------------------------------------------------------
def two_blocks(Bt, gate_w):
    from micromix_amd import SparseMoEBlock
    return SparseMoEBlock(gate_w, Bt.layers, Bt.cfg["k"]), SparseMoEBlock(gate_w, Bt.layers, Bt.cfg["k"], capturable=True)


def assert_blocks_agree(plain, capt, x, label):
    import torch
    T, H = x.shape
    want, want_logits = plain(x)
    lead = (2, T // 2) if T % 2 == 0 else (1, T)
    got, logits = capt(x)
    got3, logits3 = capt(x.reshape(*lead, H))
    got2, _ = capt(x)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want).all()) and float(want.float().abs().max()) > 0
    assert torch.equal(logits, want_logits) and torch.equal(logits3, want_logits)
    assert torch.equal(got, want), f"{label}: the capturable block differs from the default one"
    assert tuple(got3.shape) == (*lead, H) and torch.equal(got3.reshape(T, H), want) and torch.equal(got2, want), label


@pytest.mark.parametrize("T", [1, 7, 64, 65, 300])
def test_capturable_block_a_is_the_default_block(dev, built, T):
    Bt = built("A")
    cfg = Bt.cfg
    gate = t_from_bits(o.f32_to_bf16((0.05 * np.random.default_rng(T).standard_normal((cfg["E"], cfg["H"]))).astype(np.float32)), dev)
    plain, capt = two_blocks(Bt, gate)
    assert_blocks_agree(plain, capt, gen_bf16(dev, T, cfg["H"], 730 + T, "x"), f"A T={T}")


@pytest.mark.parametrize("name", CASES)
def test_capturable_block_with_scripted_routing(dev, built, name):
    cfg_id, T, counts = mb.SCRIPTED[name]
    Bt = built(cfg_id)
    cfg = Bt.cfg
    x_bits, _ = mb.scripted_x(counts, T, cfg["k"], bits_from_t(gen_bf16(dev, T, cfg["H"], 900 + T, "x")))
    plain, capt = two_blocks(Bt, t_from_bits(mb.gate_unit_bits(cfg["E"], cfg["H"]), dev))
    assert_blocks_agree(plain, capt, t_from_bits(x_bits, dev), name)


# ---- 4. capture ---------------------------------------------------------------------------------------------------------------------
def _hot(E, where):
    c = [0] * E
    for e, v in where.items():
        c[e] = v
    return tuple(c)


# T -> rows per expert of block A (E 8, k 2), the first one captured: sums are 2 T, none above T
ROUTINGS = {
    1: [_hot(8, {0: 1, 1: 1}), _hot(8, {3: 1, 7: 1}), _hot(8, {6: 1, 2: 1}), _hot(8, {7: 1, 0: 1})],
    16: [(4,) * 8, _hot(8, {0: 16, 1: 16}), _hot(8, {1: 1, 3: 15, 6: 16}), _hot(8, {7: 16, 2: 9, 4: 7})],
    # the largest group in the 16, 32, 48 and 64 tiers, other experts empty
    64: [(16,) * 8, (32, 32, 16, 16, 8, 8, 8, 8), (48, 40, 20, 10, 5, 5, 0, 0), _hot(8, {2: 64, 5: 64}), (17, 33, 49, 29, 0, 0, 0, 0)],
    # groups on both sides of 64 / 65, past 128 and 256 rows, and a call without any group above 64
    300: [(64, 65, 300, 171, 0, 0, 0, 0), (65, 64, 129, 257, 85, 0, 0, 0), _hot(8, {1: 300, 6: 300}), (75,) * 8,
          (64, 64, 64, 64, 64, 64, 64, 152), (60, 64, 61, 63, 62, 64, 64, 162)],
}


@pytest.mark.parametrize("T", sorted(ROUTINGS))
def test_one_capture_replays_on_other_routings(dev, built, T):
    import torch
    Bt = built("A")
    cfg = Bt.cfg
    E, k, H = cfg["E"], cfg["k"], cfg["H"]
    plain, capt = two_blocks(Bt, t_from_bits(mb.gate_unit_bits(E, H), dev))
    inputs = []
    for i, counts in enumerate(ROUTINGS[T]):
        bits, ids = mb.scripted_x(counts, T, k, bits_from_t(gen_bf16(dev, T, H, 750 + 10 * T + i, "x")))
        inputs.append((counts, t_from_bits(bits, dev)))
    static_in = inputs[0][1].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                             # warm-up outside the capture, as micromix_amd/graph.py does
        for _ in range(2):
            capt(static_in)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                             # a read of device data on the host would end the capture with an error
        static_out, static_logits = capt(static_in)
    for counts, x in inputs + inputs[:1]:                     # ... and back to the captured routing
        static_in.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        got, got_logits = static_out.clone(), static_logits.clone()
        want, want_logits = plain(x)
        torch.cuda.synchronize()
        assert np.array_equal(np.bincount(u8(mixedgemm.moe_route(want_logits, k)[0]).reshape(-1), minlength=E), counts), "the routing is not the scripted one"
        assert torch.equal(got_logits, want_logits)
        assert bool(torch.isfinite(want).all()) and float(want.float().abs().max()) > 0
        assert torch.equal(got, want), f"T={T}, rows per expert {counts}: the replay differs from the eager default block"


# ---- 5. launches --------------------------------------------------------------------------------------------------------------------
class CountingLib:
    """stands in for the ctypes handle: counts the calls of every mm_* entry"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("mm_"):
            return fn

        def counted(*a):
            self.calls.append(name)
            return fn(*a)
        return counted


def library_calls(monkeypatch, block, x):
    import torch
    counting = CountingLib(_lib.load())
    monkeypatch.setattr(_lib, "_lib", counting)
    try:
        block(x)
        torch.cuda.synchronize()
    finally:
        monkeypatch.undo()
    return [c for c in counting.calls if not c.endswith("_supported")]       # (queries launch nothing)


def test_launch_count_does_not_grow_with_the_experts(dev, built, monkeypatch):
    want = ["mm_moe_route", "mm_moe_plan", "mm_moe_quantize", "mm_moe_matmul", "mm_moe_matmul", "mm_moe_quantize", "mm_moe_matmul", "mm_moe_combine"]
    seen = {}
    for cfg_id, name in (("A", "A largest 16"), ("C", "C one token")):
        _, T, counts = mb.SCRIPTED[name]
        Bt = built(cfg_id)
        cfg = Bt.cfg
        x_bits, _ = mb.scripted_x(counts, T, cfg["k"], bits_from_t(gen_bf16(dev, T, cfg["H"], 900 + T, "x")))
        plain, capt = two_blocks(Bt, t_from_bits(mb.gate_unit_bits(cfg["E"], cfg["H"]), dev))
        x = t_from_bits(x_bits, dev)
        capt(x)
        seen[cfg_id] = (library_calls(monkeypatch, capt, x), library_calls(monkeypatch, plain, x))
    assert seen["A"][0] == want and seen["C"][0] == want, seen          # E = 8 and E = 64, k = 8, T = 1: the same eight calls
    assert len(seen["C"][1]) == 9                                        # (the default block: the same number of calls, but each grouped
    #                                                                      call of E = 64 is eight launches and the offsets come to the host)


# ---- operands at the end of their allocations -----------------------------------------------------------------------------------------
def test_device_sized_entries_stay_inside_their_operands():
    """tests/moe_device_sized_bounds_probe.py in a child process (a memory fault would kill it, not this run): mm_moe_quantize and
    mm_moe_matmul with every operand at the very end of a hipMalloc allocation of its own give the bytes they give on torch's pool"""
    probe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "moe_device_sized_bounds_probe.py")
    r = subprocess.run([sys.executable, probe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"the probe died (exit {r.returncode}):\n{r.stdout}\n{r.stderr[-2000:]}"
    lines = [l.split() for l in r.stdout.splitlines() if l.startswith("case")]
    assert len(lines) == 3 and "done" in r.stdout, r.stdout
    for _, label, got, want in lines:
        assert got == want, f"{label}: other bytes with the operands at the end of their allocations"
