"""Run by tests/test_add_rmsnorm_gpu.py in a child process: mm_add_rmsnorm_quantize with every operand placed at the very END of a
hipMalloc allocation of its own (whole 2 MiB pages, so the bytes behind an operand are not part of any allocation of this process), as
tests/rope_bounds_probe.py does.  One case per kernel (the products kernel, the 16-bit kernel at one and at two groups per thread).
Prints the SHA-1 of (S_out, the six buffers) for the operands at the end of their allocations and for the same call in torch's pool; a
memory fault kills this process (the parent reports it)."""
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
    assert n % 16 == 0
    size = (n + PAGE - 1) // PAGE * PAGE
    p = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(p), size) == 0
    dst = p.value + size - n
    assert hip.hipMemcpy(dst, t.data_ptr(), n, 3) == 0   # hipMemcpyDeviceToDevice
    return dst


g = torch.Generator().manual_seed(1)
st = torch.cuda.current_stream().cuda_stream
h = lambda ts: hashlib.sha1(b"".join(t.cpu().contiguous().view(torch.uint8).numpy().tobytes() for t in ts)).hexdigest()
for rows, K, split in ((3, 384, (128, 128, 128)), (3, 8320, (4096, 128, 4096)), (2, 16512, (8192, 128, 8192))):
    x = torch.randn((rows, K), generator=g).to(torch.bfloat16).to(dev)
    r = torch.randn((rows, K), generator=g).to(torch.bfloat16).to(dev)
    w = (1 + 0.1 * torch.randn((K,), generator=g)).to(torch.bfloat16).to(dev)
    idx = torch.randperm(K, generator=g).to(torch.int16).to(dev)
    want = mixedgemm.add_rmsnorm_quantize_x(x, r, w, 1e-5, idx, *split)
    torch.cuda.synchronize()
    # scale tensors: only rows' bytes are written; both runs start from zeros so that the hashes cover the same bytes
    ref = [want[0]] + [t for t in want[1:4]]
    outs = [torch.zeros_like(t) for t in want]
    plain = [torch.zeros_like(t) for t in want]
    status = lib.mm_add_rmsnorm_quantize(x.data_ptr(), r.data_ptr(), plain[0].data_ptr(), w.data_ptr(), 1e-5, rows, K, idx.data_ptr(), *split, 0,
                                         *[t.data_ptr() if t.numel() else None for t in plain[1:]], st)
    assert status == 0, status
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(plain[:4], ref))
    ptrs = [at_end(t) if t.numel() else None for t in (x, r, w, idx, *outs)]
    status = lib.mm_add_rmsnorm_quantize(ptrs[0], ptrs[1], ptrs[4], ptrs[2], 1e-5, rows, K, ptrs[3], *split, 0, *ptrs[5:], st)
    assert status == 0, status
    torch.cuda.synchronize()
    for t, p in zip(outs, ptrs[4:]):
        if t.numel():
            assert hip.hipMemcpy(t.data_ptr(), p, t.numel() * t.element_size(), 3) == 0
    torch.cuda.synchronize()
    print("case", rows, K, h(outs), h(plain), flush=True)
print("done", flush=True)
