"""Run by tests/test_moe_gpu.py in a child process: mm_moe_gather and mm_moe_combine with every operand placed at the very END of a
hipMalloc allocation of its own (whole 2 MiB pages, so the bytes behind an operand belong to no allocation of this process), as
tests/rope_bounds_probe.py does.  Prints the SHA-1 of the output for the operands at the end of their allocations and for the same
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
    assert n % 16 == 0
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


g = torch.Generator().manual_seed(2)
st = torch.cuda.current_stream().cuda_stream
rnd = lambda *shape: torch.randn(shape, generator=g).to(torch.bfloat16).to(dev)
h = lambda t: hashlib.sha1(t.cpu().view(torch.int16).numpy().tobytes()).hexdigest()
T, K, E = 8, 2, 4         # every operand a whole number of 16-byte pieces
for H in (8, 384, 4096):
    x = rnd(T, H)
    ids = torch.stack([torch.randperm(E, generator=g)[:K] for _ in range(T)]).to(torch.int32).to(dev)
    w = torch.rand((T, K), generator=g).to(torch.bfloat16).to(dev)
    _, sorted_token, slot_of = mixedgemm.moe_plan(ids, E)           # T * K = 16 pairs: the last sorted row is the last row of x_sorted
    want_g = mixedgemm.moe_gather(x, sorted_token)
    want_c = mixedgemm.moe_combine(want_g, ids, w, slot_of)
    torch.cuda.synchronize()
    p = {n: at_end(t) for n, t in dict(x=x, tok=sorted_token, xs=torch.zeros_like(want_g), ids=ids, w=w,
                                       slot=slot_of, out=torch.zeros_like(want_c)).items()}
    assert lib.mm_moe_gather(p["x"], p["tok"], T, T * K, H, p["xs"], st) == 0
    assert lib.mm_moe_combine(p["xs"], p["ids"], p["w"], p["slot"], T, K, H, p["out"], st) == 0
    torch.cuda.synchronize()
    got_g, got_c = fetch(torch.empty_like(want_g), p["xs"]), fetch(torch.empty_like(want_c), p["out"])
    print("case", H, h(got_g) + h(got_c), h(want_g) + h(want_c), flush=True)
print("done", flush=True)
