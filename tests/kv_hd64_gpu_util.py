"""What the GPU tests of the 64-wide paged cache share (tests/test_kv_exact_hd64_gpu.py, test_kv_edges_hd64_gpu.py): tensors from the numpy
arrays of tests/kv_exact_cases_hd64.py, a poisoned device cache, its filling through the library's own append, and the row check."""
import numpy as np
import torch

from micromix_amd import mixedgemm
import kv_exact_cases_hd64 as k6

KINDS = ("bf16", "fp8")
L, LAYER = 3, 1


def i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def bf(x, dev):
    """float32 numpy holding bf16 values -> bf16 tensor (exact)"""
    k6.bf16_bits(x)
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).to(dev)


def f64(o):
    return o.float().cpu().numpy().astype(np.float64)


def device_cache(kind, max_pages, Hkv, P, dev, poison=True, layers=L):
    hd, hp = k6.empty_host_cache(kind, max_pages, layers, Hkv, P, poison)
    if kind == "bf16":
        return torch.from_numpy(hd.view(np.int16)).to(dev).view(torch.bfloat16), None
    return torch.from_numpy(hd).to(dev).view(torch.float8_e4m3fn), torch.from_numpy(hp).to(dev)


def fill(kind, K, V, lens, P, dev, seed=0, rope=False, poison=True):
    """a poisoned cache of L layers whose layer LAYER holds the sequences' K / V, appended by the library"""
    indptr, indices, last, max_pages = k6.page_table(lens, P, seed)
    assert not (indices == 0).any(), "page 0 must stay unreferenced: masked tokens form their addresses from row 0"
    data, param = device_cache(kind, max_pages, K.shape[1], P, dev, poison)
    tbl, app, k, v = [i32(a, dev) for a in (indptr, indices, last)], i32(k6.indptr_of(lens), dev), bf(K, dev), bf(V, dev)
    if rope:
        one = torch.ones((k.size(0), 64), dtype=torch.bfloat16, device=dev)
        assert torch.equal(mixedgemm.rope_kv_append(data, param, *tbl, k, k, v, one, torch.zeros_like(one), app, LAYER), k)
    else:
        mixedgemm.kv_append(data, param, *tbl, k, v, app, LAYER)
    return dict(data=data, param=param, tbl=tbl, tbl_h=(indptr, indices, last), pages=indices, P=P, max_pages=max_pages)


def expect_rows(o, want, labels, bound, what, grid=True):
    """asserts |o - want| <= bound row by row (a failure names the row and, grid, the token it holds); returns the worst error / bound"""
    got = f64(o).reshape(-1, 64)
    msg = k6.describe_mismatch(got, want.reshape(-1, 64), labels, bound, grid)
    assert msg is None, f"{what}: {msg}"
    err = np.abs(got - want.reshape(-1, 64)) / np.maximum(bound, 1e-300)
    return float(np.where(np.broadcast_to(np.asarray(bound) > 0, err.shape), err, 0.0).max())
