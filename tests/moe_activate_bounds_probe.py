"""Run by tests/test_moe_activate_gpu.py in a child process: mm_moe_activate_quantize with every operand -- a, b, h_out, the offsets, the
expert table, the reorder indices it points to, all six outputs -- placed at the very END of a hipMalloc allocation of its own (whole
2 MiB pages, so the bytes behind an operand belong to no allocation of this process), as tests/moe_device_sized_bounds_probe.py does
for the other device-sized entries.  Prints the SHA-1 of the outputs for the operands at the end of their allocations and for the same
bytes in torch's pool; a memory fault kills this process (the parent reports it)."""
import ctypes, hashlib, sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from micromix_amd import _lib, mixedgemm
lib = _lib.load(); dev = torch.device("cuda:0")
hip = ctypes.CDLL("libamdhip64.so")
hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
PAGE = 2 << 20


def at_end(t):
    """device address of a copy of tensor t whose last byte is the last byte of a fresh hipMalloc allocation (whole pages)"""
    n = t.numel() * t.element_size()
    assert n % 16 == 0 and n > 0
    size = (n + PAGE - 1) // PAGE * PAGE
    p = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(p), size) == 0
    dst = p.value + size - n
    assert hip.hipMemcpy(dst, t.data_ptr(), n, 3) == 0   # hipMemcpyDeviceToDevice
    return dst


def fetch(t, ptr):
    assert hip.hipMemcpy(t.data_ptr(), ptr, t.numel() * t.element_size(), 3) == 0
    torch.cuda.synchronize()
    return t


g = torch.Generator().manual_seed(5)
st = torch.cuda.current_stream().cuda_stream
rnd = lambda *shape: torch.randn(shape, generator=g).to(torch.bfloat16).to(dev)
h = lambda ts: hashlib.sha1(b"".join(t.cpu().contiguous().view(torch.uint8).numpy().tobytes() for t in ts)).hexdigest()
E, N = 3, 64                                        # (E + 1) offsets = 16 bytes; every operand a whole number of 16-byte pieces
for counts, K, split in (((5, 0, 11), 384, (128, 128, 128)), ((16, 0, 0), 384, (128, 128, 128)), ((65, 15, 0), 128, (0, 128, 0)),
                         ((3, 0, 5), 14336, (12288, 1024, 1024))):          # the last one: the 1024-thread variant
    idx = [torch.randperm(K, generator=g).to(torch.int16).to(dev) for _ in range(E)]
    Bs = [mixedgemm.reorder_quantize_w4(rnd(N, K) * 0.1, i, *split) for i in idx]
    table = mixedgemm.moe_expert_table(idx, Bs, *split)
    # the same table with the reorder indices (all this entry reads through it) at the end of an allocation
    p_table = at_end(torch.tensor([[at_end(i)] + [0] * 7 for i in idx], dtype=torch.int64).to(dev))
    n = sum(counts)
    offsets = torch.tensor([0, counts[0], counts[0] + counts[1], n], dtype=torch.int32, device=dev)
    a, b = rnd(n, K) * 2, rnd(n, K)
    want_h = torch.zeros_like(a)
    want_q = mixedgemm.moe_activate_quantize(a, b, offsets, table, h_out=want_h,
                                             out=tuple(torch.zeros_like(t) for t in mixedgemm.moe_activate_quantize(a, b, offsets, table)))
    torch.cuda.synchronize()
    po = [at_end(torch.zeros_like(t)) if t.numel() else None for t in want_q]
    p_a, p_b, p_h, p_off = at_end(a), at_end(b), at_end(torch.zeros_like(want_h)), at_end(offsets)
    assert lib.mm_moe_activate_quantize(p_a, p_b, p_off, p_table, E, n, K, *split, *po, p_h, st) == 0
    torch.cuda.synchronize()
    got_q = [fetch(torch.empty_like(t), p) if t.numel() else t for t, p in zip(want_q, po)]
    got_h = fetch(torch.empty_like(want_h), p_h)
    print("case", "-".join(map(str, counts)) + f"-K{K}", h(got_q + [got_h]), h(list(want_q) + [want_h]), flush=True)
print("done", flush=True)
