"""CPU tests of mm_moe_gate_up_activate (include/micromix_hip.h) and of the packed w1 | w3 weight behind it: the entries exist while
mm_version stays 660, every argument error is answered without device work, mixedgemm.permute_packed_rows is a byte shuffle equal to
quantizing the row-permuted weight with the oracle's w4 quantizer, and mixedgemm.moe_gate_up_table refuses what the fused launch has
no kernel for before it touches a device."""
import numpy as np
import pytest
import torch

from micromix_amd import _lib, mixedgemm
from oracle import mx_oracle as o


def test_entries_exist_and_the_version_stays():
    lib = _lib.load()
    for name in ("mm_moe_gate_up_activate", "mm_moe_gate_up_activate_supported"):
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert lib.mm_version() == 660
    for name in ("permute_packed_rows", "moe_gate_up_table", "moe_gate_up_activate", "moe_gate_up_activate_supported"):
        assert name in mixedgemm.__all__ and callable(getattr(mixedgemm, name)), name


def test_status_codes_without_device_work():
    lib = _lib.load()
    z, p = None, 16                                           # p: a non-null, 16-byte aligned pointer that is never dereferenced here
    S, U, B, OK = _lib.MM_ERR_BAD_SPLIT, _lib.MM_ERR_UNSUPPORTED, _lib.MM_ERR_BAD_ARG, _lib.MM_OK
    gu = lambda a3=(p, p, p), sfa3=(p, p, p), off=p, tab=p, E=8, n=16, max_rows=16, I=384, split1=(128, 128, 128), split2=(128, 128, 128), flags=0, \
        o3=(p, p, p), sf3=(p, p, p): lib.mm_moe_gate_up_activate(*a3, *sfa3, off, tab, E, n, max_rows, I, *split1, *split2, flags, *o3, *sf3, z)
    # null operands
    assert gu(a3=(z, p, p)) == B and gu(a3=(p, p, z)) == B and gu(sfa3=(p, z, p)) == B and gu(off=z) == B and gu(tab=z) == B
    assert gu(o3=(z, p, p)) == B and gu(o3=(p, p, z)) == B and gu(sf3=(z, p, p)) == B and gu(sf3=(p, p, z)) == B
    assert gu(tab=12) == B and gu(o3=(8, p, p)) == B and gu(sf3=(p, 4, p)) == B                  # misaligned
    for E in (0, 65, 1000):                                   # E outside 1 .. 64
        assert gu(E=E) == U, E
    assert gu(E=-1) == B and gu(n=-1) == B and gu(I=-384) == B
    assert gu(I=400, split2=(128, 128, 144)) == S and gu(I=100, split2=(100, 0, 0)) == S          # I % 128 != 0
    assert gu(split2=(128, 192, 64)) == S and gu(split2=(128, 128, 0)) == S                       # a split2 entry not in 128s / not adding up to I
    assert gu(split1=(128, 100, 28)) == S and gu(split1=(0, 0, 0)) == S
    assert gu(max_rows=0) == B and gu(max_rows=-5) == B       # max_rows < 1
    assert gu(flags=_lib.MM_OUT_F32) == B and gu(flags=_lib.MM_SPLIT_K_ALWAYS) == B
    assert gu(a3=(z, z, z), sfa3=(z, z, z), off=z, tab=z, n=0, o3=(z, z, z), sf3=(z, z, z)) == OK      # n = 0, whatever the pointers
    sup = lib.mm_moe_gate_up_activate_supported
    assert sup(16, 384, 128, 128, 128, 128, 128, 128, _lib.MM_W_FP4) == 1
    assert sup(16, 384, 128, 128, 128, 128, 128, 128, _lib.MM_W_MATCH) == 0                       # the "w" weight mode
    assert sup(16, 384, 128, 0, 0, 128, 128, 128, _lib.MM_W_MATCH) == 1                           # (one fp4 segment: fp4 weights in both modes)
    assert sup(0, 384, 128, 128, 128, 128, 128, 128, _lib.MM_W_FP4) == 0 and sup(16, 400, 128, 128, 128, 128, 128, 144, _lib.MM_W_FP4) == 0
    assert sup(16, 384, 128, 128, 128, 128, 192, 64, _lib.MM_W_FP4) == 0 and sup(16, 384, 128, 128, 128, 128, 128, 128, 7) == 0


N, K, SPLIT = 256, 384, (128, 128, 128)


@pytest.fixture(scope="module")
def weight():
    rng = np.random.default_rng(11)
    w = o.f32_to_bf16((0.3 * rng.standard_normal((N, K)) * np.exp2(rng.integers(-6, 6, size=(N, 1)))).astype(np.float32))
    return w, rng.permutation(K)


def pack(w_bits, idx):
    return tuple(torch.from_numpy(np.ascontiguousarray(t)) for t in o.reorder_quantize(w_bits, idx, *SPLIT, "w4"))


@pytest.mark.parametrize("which", ["identity", "reversal", "random"])
def test_permute_packed_rows_is_the_quantization_of_the_permuted_weight(weight, which):
    w, idx = weight
    perm = {"identity": np.arange(N), "reversal": np.arange(N)[::-1].copy(), "random": np.random.default_rng(3).permutation(N)}[which]
    packed = pack(w, idx)
    got = mixedgemm.permute_packed_rows(packed, torch.from_numpy(perm))
    want = pack(w[perm], idx)
    for i, (g, t) in enumerate(zip(got, want)):
        assert g.dtype == torch.uint8 and g.shape == t.shape and torch.equal(g, t), f"{which}: tensor {i} of the packed 6-tuple"
    if which != "identity":
        assert not torch.equal(got[0], packed[0]) and not torch.equal(got[3], packed[3])
    # ... an int16 index, as the layers hold theirs, and the gate / up interleave on top of it round-trips
    got16 = mixedgemm.permute_packed_rows(packed, torch.from_numpy(perm.astype(np.int16)))
    assert all(torch.equal(a, b) for a, b in zip(got16, got))
    gate, up = mixedgemm.deinterleave_gate_up(mixedgemm.interleave_gate_up(got, packed))
    assert all(torch.equal(a, b) for a, b in zip(gate, got)) and all(torch.equal(a, b) for a, b in zip(up, packed))


def test_permute_packed_rows_refuses_what_is_no_permutation(weight):
    w, idx = weight
    packed = pack(w, idx)
    with pytest.raises(ValueError):
        mixedgemm.permute_packed_rows(packed, torch.zeros(N, dtype=torch.long))
    with pytest.raises(ValueError):
        mixedgemm.permute_packed_rows(packed, torch.arange(N - 1))
    with pytest.raises(ValueError):
        mixedgemm.permute_packed_rows(tuple(t[:100] if t.dim() == 2 else t for t in packed), torch.arange(100))


def test_gate_up_table_refuses_biases_w_weights_and_bad_splits(weight):
    E, H, I = 2, 384, 256
    w, idx1 = weight                                          # [I = 256, H = 384]
    idx2 = [torch.from_numpy(np.random.default_rng(e).permutation(I).astype(np.int16)) for e in range(E)]
    i1 = [torch.from_numpy(idx1.astype(np.int16))] * E
    w4 = [pack(w, idx1)] * E
    wm = [tuple(torch.from_numpy(np.ascontiguousarray(t)) for t in o.reorder_quantize(w, idx1, *SPLIT, "w"))] * E
    bias = [torch.zeros(I, dtype=torch.bfloat16)] * E
    with pytest.raises(ValueError, match="bias"):
        mixedgemm.moe_gate_up_table(i1, w4, w4, idx2, SPLIT, (128, 128, 0), biases1=bias)
    with pytest.raises(ValueError, match="bias"):
        mixedgemm.moe_gate_up_table(i1, w4, w4, idx2, SPLIT, (128, 128, 0), biases3=[None, bias[0]])
    with pytest.raises(ValueError, match="fp4"):
        mixedgemm.moe_gate_up_table(i1, wm, wm, idx2, SPLIT, (128, 128, 0))
    with pytest.raises(ValueError, match="fp4"):
        mixedgemm.moe_gate_up_table(i1, w4, wm, idx2, SPLIT, (128, 128, 0))
    with pytest.raises(ValueError, match="split2"):
        mixedgemm.moe_gate_up_table(i1, w4, w4, idx2, SPLIT, (192, 64, 0))
    with pytest.raises(ValueError, match="split2"):
        mixedgemm.moe_gate_up_table(i1, w4, w4, idx2, SPLIT, (128, 0, 0))
    odd = [tuple(t[:200] if t.dim() == 2 else t for t in w4[0])] * E                  # I = 200
    with pytest.raises(ValueError, match="multiple of 128"):
        mixedgemm.moe_gate_up_table(i1, odd, odd, idx2, SPLIT, (128, 72, 0))
