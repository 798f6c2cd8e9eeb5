"""Run by tests/test_moe_device_sized_gpu.py in a child process: mm_moe_quantize and mm_moe_matmul with every operand -- rows, row
indices, offsets, the expert table, the weights it points to, all outputs -- placed at the very END of a hipMalloc allocation of its
own (whole 2 MiB pages, so the bytes behind an operand belong to no allocation of this process), as tests/moe_bounds_probe.py does for
the other MoE entries.  Prints the SHA-1 of the outputs for the operands at the end of their allocations and for the same bytes in
torch's pool; a memory fault kills this process (the parent reports it)."""
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


g = torch.Generator().manual_seed(3)
st = torch.cuda.current_stream().cuda_stream
rnd = lambda *shape: torch.randn(shape, generator=g).to(torch.bfloat16).to(dev)
h = lambda ts: hashlib.sha1(b"".join(t.cpu().contiguous().view(torch.uint8).numpy().tobytes() for t in ts)).hexdigest()
E, K, N, split = 3, 256, 64, (128, 0, 128)        # (E + 1) offsets = 16 bytes; every operand a whole number of 16-byte pieces
idx = [torch.randperm(K, generator=g).to(torch.int16).to(dev) for _ in range(E)]
Bs = [mixedgemm.reorder_quantize_w4(rnd(N, K) * 0.1, i, *split) for i in idx]
bias = [rnd(N), None, rnd(N)]
table = mixedgemm.moe_expert_table(idx, Bs, *split, biases=bias)
# the same table with every tensor it points to at the end of an allocation (segment S is empty: its pointers stay null)
rows = [[at_end(i)] + [at_end(t) if t.numel() else 0 for t in B] + [at_end(b) if b is not None else 0] for i, B, b in zip(idx, Bs, bias)]
p_table = at_end(torch.tensor(rows, dtype=torch.int64).to(dev))
for counts in ((5, 0, 11), (16, 0, 0), (65, 15, 0)):
    n = sum(counts)
    T = n                                           # every slot reads a row of its own, the last slot the last row of src
    offsets = torch.tensor([0, counts[0], counts[0] + counts[1], n], dtype=torch.int32, device=dev)
    row_of_slot = torch.randperm(n, generator=g).to(torch.int32).to(dev)
    row_of_slot[n - 1] = T - 1
    src = rnd(T, K)
    want_q = mixedgemm.moe_quantize(src, row_of_slot, offsets, table, out=tuple(torch.zeros_like(t) for t in mixedgemm.moe_quantize(src, row_of_slot, offsets, table)))
    want_d = mixedgemm.moe_matmul(want_q, offsets, table, n, out=torch.zeros((n, N), dtype=torch.bfloat16, device=dev))
    torch.cuda.synchronize()
    po = [at_end(torch.zeros_like(t)) if t.numel() else None for t in want_q]
    p_src, p_ros, p_off, p_d = at_end(src), at_end(row_of_slot), at_end(offsets), at_end(torch.zeros_like(want_d))
    assert lib.mm_moe_quantize(p_src, p_ros, p_off, p_table, E, n, T, K, *split, _lib.MM_QUANT_MIXED, *po, st) == 0
    assert lib.mm_moe_matmul(*po, p_off, p_table, E, n, n, N, *split, _lib.MM_W_FP4, 0, p_d, st) == 0
    torch.cuda.synchronize()
    got_q = [fetch(torch.empty_like(t), p) if t.numel() else t for t, p in zip(want_q, po)]
    got_d = fetch(torch.empty_like(want_d), p_d)
    print("case", "-".join(map(str, counts)), h(got_q + [got_d]), h(list(want_q) + [want_d]), flush=True)
print("done", flush=True)
