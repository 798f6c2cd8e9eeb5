"""Run by tests/test_moe_gate_up_gpu.py in a child process: mm_moe_gate_up_activate with every operand -- the six quantized activation
buffers, the offsets, the expert table, the six packed w1 | w3 tensors of every expert that it points to, all six outputs -- placed at
the very END of a hipMalloc allocation of its own (whole 2 MiB pages, so the bytes behind an operand belong to no allocation of this
process), as tests/moe_activate_bounds_probe.py does for the activation quantizer.  Prints the SHA-1 of the outputs for the operands
at the end of their allocations and for the same bytes in torch's pool; a memory fault kills this process (the parent reports it)."""
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


g = torch.Generator().manual_seed(7)
st = torch.cuda.current_stream().cuda_stream
rnd = lambda *shape: torch.randn(shape, generator=g).to(torch.bfloat16).to(dev)
h = lambda ts: hashlib.sha1(b"".join(t.cpu().contiguous().view(torch.uint8).numpy().tobytes() for t in ts)).hexdigest()
E = 3                                               # (E + 1) offsets = 16 bytes; every operand a whole number of 16-byte pieces
for counts, H, split1, I, split2 in (((5, 0, 11), 384, (128, 128, 128), 384, (128, 128, 128)), ((65, 15, 0), 128, (0, 0, 128), 256, (0, 128, 128)),
                                     ((130, 0, 1), 256, (128, 0, 128), 128, (128, 0, 0)), ((0, 0, 257), 128, (128, 0, 0), 256, (128, 128, 0))):
    idx1 = [torch.randperm(H, generator=g).to(torch.int16).to(dev) for _ in range(E)]
    idx2 = [torch.randperm(I, generator=g).to(torch.int16).to(dev) for _ in range(E)]
    w1s = [mixedgemm.reorder_quantize_w4(rnd(I, H) * 0.3, i, *split1) for i in idx1]
    w3s = [mixedgemm.reorder_quantize_w4(rnd(I, H) * 0.3, i, *split1) for i in idx1]
    table = mixedgemm.moe_gate_up_table(idx1, w1s, w3s, idx2, split1, split2)
    # the same table with every tensor it points to at the end of an allocation (the reorder index is not read by this entry)
    rows = table.tensor.cpu().tolist()
    p_table = at_end(torch.tensor([[0] + [at_end(t) if t.numel() else 0 for t in keep[1]] + [0] for keep in table._keep], dtype=torch.int64).to(dev))
    assert len(rows) == E
    n = sum(counts)
    offsets = torch.tensor([0, counts[0], counts[0] + counts[1], n], dtype=torch.int32, device=dev)
    q1 = mixedgemm.moe_quantize(rnd(n, H), None, offsets, table, out=tuple(torch.zeros_like(t) for t in mixedgemm.moe_quantize(rnd(n, H), None, offsets, table)))
    zeros = lambda: tuple(torch.zeros_like(t) for t in mixedgemm.moe_gate_up_activate(q1, offsets, table, n, split2))
    want = mixedgemm.moe_gate_up_activate(q1, offsets, table, n, split2, out=zeros())
    torch.cuda.synchronize()
    pa = [at_end(t) if t.numel() else None for t in q1]
    po = [at_end(torch.zeros_like(t)) if t.numel() else None for t in want]
    assert lib.mm_moe_gate_up_activate(*pa, at_end(offsets), p_table, E, n, n, I, *split1, *split2, 0, *po, st) == 0
    torch.cuda.synchronize()
    got = [fetch(torch.empty_like(t), p) if t.numel() else t for t, p in zip(want, po)]
    print("case", "-".join(map(str, counts)) + f"-H{H}-I{I}", h(got), h(list(want)), flush=True)
print("done", flush=True)
