"""Run by tests/test_rope_append_gpu.py in a child process: mm_rope_kv_append at T = 1 with every operand placed at the very END of a
hipMalloc allocation of its own (whole 2 MiB pages, so the bytes behind an operand are not part of any allocation of this process), as
tests/bounds_probe.py does for the weight-streaming kernel.  Prints the SHA-1 of (q_rot, cache) for the operands at the end of their
allocations and for the same bytes in torch's pool; a memory fault kills this process (the parent reports it)."""
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
    assert n % 4 == 0
    size = (n + PAGE - 1) // PAGE * PAGE
    p = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(p), size) == 0
    dst = p.value + size - n
    assert hip.hipMemcpy(dst, t.data_ptr(), n, 3) == 0   # hipMemcpyDeviceToDevice
    return dst


g = torch.Generator().manual_seed(1)
st = torch.cuda.current_stream().cuda_stream
Hq, Hkv, P, L, max_pages = 32, 8, 16, 2, 3
rnd = lambda *shape: torch.randn(shape, generator=g).to(torch.bfloat16).to(dev)
i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)
h = lambda *ts: hashlib.sha1(b"".join(t.cpu().view(torch.int16).numpy().tobytes() for t in ts)).hexdigest()
for kind in (0, 1):
    q, k, v, cos, sin = rnd(1, Hq, 128), rnd(1, Hkv, 128), rnd(1, Hkv, 128), rnd(1, 128), rnd(1, 128)
    # the token goes to the last slot of the last page: the cache rows written are the last of K and of V of layer 1's last head too
    indptr, indices, last, app = i32([0, 2]), i32([0, max_pages - 1]), i32([P]), i32([0, 1])
    if kind == 0:
        data = torch.zeros((max_pages, L, 2, Hkv, P, 64), dtype=torch.uint8, device=dev)
        param = torch.zeros((max_pages, L, 2, Hkv, P, 2), dtype=torch.float16, device=dev)
    else:
        data, param = torch.zeros((max_pages, L, 2, Hkv, P, 128), dtype=torch.bfloat16, device=dev), None
    want_q = mixedgemm.rope_kv_append(data, param, indptr, indices, last, q, k, v, cos, sin, app, L - 1)
    torch.cuda.synchronize()
    want = h(want_q, data.view(torch.int16), *([param] if param is not None else []))
    data.zero_()
    out = torch.zeros_like(want_q)
    if param is not None:
        param.zero_()
    ptrs = {n: at_end(t) for n, t in dict(q=q, k=k, v=v, cos=cos, sin=sin, indptr=indptr, indices=indices, last=last, app=app, out=out,
                                           data=data, **({"param": param} if param is not None else {})).items()}
    status = lib.mm_rope_kv_append(ptrs["data"], ptrs.get("param"), kind, max_pages, L, L - 1, Hkv, P, 128, ptrs["indptr"], ptrs["indices"],
                                   ptrs["last"], 1, ptrs["q"], ptrs["k"], ptrs["v"], Hq * 128, Hq, ptrs["cos"], ptrs["sin"], 128, ptrs["app"], 1,
                                   ptrs["out"], st)
    assert status == 0, status
    torch.cuda.synchronize()
    for n, t in (("out", out), ("data", data)) + ((("param", param),) if param is not None else ()):
        assert hip.hipMemcpy(t.data_ptr(), ptrs[n], t.numel() * t.element_size(), 3) == 0
    torch.cuda.synchronize()
    print("case", kind, h(out, data.view(torch.int16), *([param] if param is not None else [])), want, flush=True)
print("done", flush=True)
