"""`mixedgemm` -- drop-in for the reference's pybind11 extension of the same name
(mgemm/src/bindings.cpp:682-742), MX hot path only, backed by libmicromix_hip.so.

Same function names, argument order, keyword names, return tuples, dtypes and shapes:

    matmul(AN, BN, AS, BS, AO, BO, SFAN, SFBN, SFAS, SFBS, SFAO, SFBO) -> Tensor[M, N] bf16
    reorder_quantize_x(X, reorder_index, KN, KS, KO)  -> (XN, XS, XO, SFXN, SFXS, SFXO)
    reorder_quantize_w(W, reorder_index, KN, KS, KO)  -> (WN, WS, WO, SFWN, SFWS, SFWO)
    reorder_quantize_w4(W, reorder_index, KN, KS, KO) -> (WN, WS, WO, SFWN, SFWS, SFWO)
    activate_quantize_x(A, B, KN, KS, KO)             -> (XN, XS, XO, SFXN, SFXS, SFXO)   (section 8f rank 1)
    downproj_quantize_w / _w4 (W, KN, KS, KO)         -> (WN, WS, WO, SFWN, SFWS, SFWO)
    rmsnorm_quantize_x(X, W, eps, reorder_index, KN, KS, KO) -> (XN, XS, XO, SFXN, SFXS, SFXO)    (section 8f rank 2)

Differences from the reference, all deliberate:
  * kernels are queued on torch's CURRENT stream of the tensors' device (the reference uses
    the legacy default stream and no device guard, reorder.cu:455, w4a4.cu:182);
  * any K that is a multiple of 128 (<= 32768) works, not only the ten compiled-in values
    (bindings.cpp:134-148); bad splits still raise RuntimeError("Value error in run_...");
  * inputs are validated (dtype/device/contiguity) instead of being reinterpreted blindly;
  * `matmul` takes optional keyword-only `bias` and `rounding` arguments (extensions).
The remaining exports of the reference module (FlashInfer KV ops) are outside the hot path; they raise
NotImplementedError.  The paged KV cache itself is `kv_append` / `paged_decode` / `paged_prefill` below (GQA, bf16 q,
quantizes K/V itself; micromix_amd/kvcache.py wraps them), on the reference's FlashInfer layout.
"""
from __future__ import annotations

import torch

from . import _lib

__all__ = ["test_function", "matmul", "gate_up_activate", "interleave_gate_up", "reorder_quantize_x", "reorder_quantize_w", "reorder_quantize_w4", "activate_quantize_x",
           "downproj_quantize_w", "downproj_quantize_w4", "rmsnorm_quantize_x", "qlinear_decode", "qlinear_decode_supported", "matmul_grouped", "reorder_quantize_x_grouped",
           "kv_append", "rope_kv_append", "kv_copy_pages", "kv_move_rows", "paged_decode", "paged_decode_workspace_bytes", "paged_decode_shared", "paged_decode_shared_workspace_bytes", "paged_prefill", "paged_prefill_workspace_bytes",
           "argmax_rows", "argmax_rows_workspace_bytes", "verify_greedy", "sample_rows", "sample_rows_workspace_bytes",
           "moe_route", "moe_plan", "moe_gather", "moe_combine",
           "moe_expert_table", "moe_sf_bytes", "moe_quantize", "moe_activate_quantize", "moe_matmul", "moe_matmul_supported",
           "permute_packed_rows", "moe_gate_up_table", "moe_gate_up_activate", "moe_gate_up_activate_supported"]


def test_function():
    """bindings.cpp:700: the module's liveness probe (answered by the HIP library, so it also proves the library loads)."""
    return _lib.load().mm_test_function().decode()


def _stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _check_tensor(t, name, dtype, device=None):
    """Slow path: produces the precise error.  The ops call it only after the cheap combined test failed."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a device tensor (HIP); the MicroMix ops have no CPU path")
    if device is not None and t.device != device:
        raise RuntimeError(f"{name} is on {t.device}, expected {device}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")


def _ok(t, dtype, index) -> bool:
    # one short-circuit expression per tensor: ~0.3 us instead of ~0.7 us for the descriptive checks
    return t.dtype is dtype and t.is_cuda and t.get_device() == index and t.is_contiguous()


def _ptr(t):
    return t.data_ptr() if t.numel() else None


def _sf_bytes_x(m, k):   # bindings.cpp:120-123
    return (m // 128 + 1) * 128 * (k // 32)


def _sf_bytes_w(n, k):   # bindings.cpp:170-172 (rows padded to 128)
    return (n + 127) // 128 * 128 * (k // 32)


def _check_split(KN, KS, KO, K, what):
    """the reference's "Value error in run_<what>" unless (KN, KS, KO) are non-negative multiples of 128 that add up to K (K None: to
    anything but 0)"""
    if KN < 0 or KS < 0 or KO < 0 or KN % 128 or KS % 128 or KO % 128 or (KN + KS + KO != K if K is not None else KN + KS + KO == 0):
        _lib.check(_lib.MM_ERR_BAD_SPLIT, what)


def _round_flags(rounding, integer_round=True):
    if rounding not in ("reference", "fused"):
        raise ValueError("rounding must be 'reference' or 'fused'")
    return (_lib.MM_ROUND_PER_SEGMENT if rounding == "reference" else _lib.MM_ROUND_ONCE) | (0 if integer_round else _lib.MM_NORM_NO_INTEGER_ROUND)


def _weight_mode(B, N, KN, KS, KO, split_name="(KN, KS, KO)"):
    """the weight mode of packed weights B = (BN, BS, BO, ...) of N rows, read off their widths: matching precision or all fp4"""
    same = B[1].size(1) == KS // 4 * 3 and B[2].size(1) == KO
    w4 = B[1].size(1) == KS // 2 and B[2].size(1) == KO // 2
    if B[0].size(1) != KN // 2 or not (same or w4) or B[1].size(0) != N or B[2].size(0) != N:
        raise RuntimeError(f"packed weights do not match {split_name}")
    return _lib.MM_W_MATCH if same else _lib.MM_W_FP4


def _check_weight_scales(SF, N, KN, KS, KO, names=None):
    """the scale tensors SF of N rows hold enough bytes; names: say which one does not"""
    if SF[0].numel() < _sf_bytes_w(N, KN) or SF[1].numel() < _sf_bytes_w(N, KS) or SF[2].numel() < _sf_bytes_w(N, KO):
        for n, t, k in zip(names or (), SF, (KN, KS, KO)):
            if t.numel() < _sf_bytes_w(N, k):
                raise RuntimeError(f"{n} holds {t.numel()} scale bytes, needs at least {_sf_bytes_w(N, k)}")
        raise RuntimeError("weight scale tensors are too small")


class _on_device:
    """`with torch.cuda.device(d)` only when d is not already current (saves ~2 us per call)."""
    __slots__ = ("idx", "prev")

    def __init__(self, idx):
        self.idx = idx
        self.prev = -1

    def __enter__(self):
        cur = torch.cuda.current_device()
        if cur != self.idx:
            self.prev = cur
            torch.cuda.set_device(self.idx)

    def __exit__(self, *exc):
        if self.prev >= 0:
            torch.cuda.set_device(self.prev)
        return False


def _quantize(src, reorder_index, KN, KS, KO, mode, what, gather_subset=False):
    lib = _lib.load()
    if not (isinstance(src, torch.Tensor) and isinstance(reorder_index, torch.Tensor) and src.is_cuda
            and _ok(src, torch.bfloat16, src.get_device()) and _ok(reorder_index, torch.int16, src.get_device())):
        _check_tensor(src, "X" if mode == "x" else "W", torch.bfloat16)
        _check_tensor(reorder_index, "reorder_index", torch.int16, src.device)
    if src.dim() != 2:
        raise RuntimeError("input must be 2-D [rows, K]")
    KN, KS, KO = int(KN), int(KS), int(KO)
    rows, K = src.shape
    if reorder_index.numel() != KN + KS + KO or (gather_subset and (K % 128 or KN + KS + KO > K)):
        _lib.check(_lib.MM_ERR_BAD_SPLIT, what)
    if KN < 0 or KS < 0 or KO < 0 or KN % 128 or KS % 128 or KO % 128 or (KN + KS + KO == 0 if gather_subset else KN + KS + KO != K):
        _check_split(KN, KS, KO, None if gather_subset else K, what)
    dev = src.device
    w4 = mode == "w4"
    sf_bytes = _sf_bytes_x if mode == "x" else _sf_bytes_w
    u8 = torch.uint8
    oN = torch.empty((rows, KN // 2), dtype=u8, device=dev)
    oS = torch.empty((rows, KS // 2 if w4 else KS // 4 * 3), dtype=u8, device=dev)
    oO = torch.empty((rows, KO // 2 if w4 else KO), dtype=u8, device=dev)
    sfN = torch.empty((sf_bytes(rows, KN),), dtype=u8, device=dev)
    sfS = torch.empty((sf_bytes(rows, KS),), dtype=u8, device=dev)
    sfO = torch.empty((sf_bytes(rows, KO),), dtype=u8, device=dev)
    with _on_device(dev.index):
        entry = lib.mm_reorder_quantize_gather if gather_subset else lib.mm_reorder_quantize
        st = entry(
            _ptr(src), rows, K, _ptr(reorder_index), KN, KS, KO,
            _lib.MM_QUANT_W4 if w4 else _lib.MM_QUANT_MIXED,
            _ptr(oN), _ptr(oS), _ptr(oO), _ptr(sfN), _ptr(sfS), _ptr(sfO), _stream_ptr(dev))
    if st:
        _lib.check(st, what)
    return oN, oS, oO, sfN, sfS, sfO


def reorder_quantize_x(X, reorder_index, KN, KS, KO):
    """bindings.cpp:104-151.  X [M,K] bf16 -> XN [M,KN/2], XS [M,3KS/4], XO [M,KO] + 3 SF tensors."""
    return _quantize(X, reorder_index, KN, KS, KO, "x", "reorder_quantize_x")


def reorder_quantize_w(W, reorder_index, KN, KS, KO):
    """bindings.cpp:155-202.  W [N,K] bf16 -> WN [N,KN/2], WS [N,3KS/4], WO [N,KO] + 3 SF tensors."""
    return _quantize(W, reorder_index, KN, KS, KO, "w", "reorder_quantize_w")


def reorder_quantize_w4(W, reorder_index, KN, KS, KO):
    """bindings.cpp:206-253.  W [N,K] bf16 -> WN [N,KN/2], WS [N,KS/2], WO [N,KO/2] + 3 SF tensors."""
    return _quantize(W, reorder_index, KN, KS, KO, "w4", "reorder_quantize_w4")


_SPLIT_WS = {}             # (device index, stream handle) -> workspace tensor; insertion order = age
_SPLIT_WS_MAX = 8          # eager workspaces kept alive at once (8-128 MiB each): the oldest stream's is released beyond that


def split_workspace(dev, nbytes):
    """The split-K scratch for a launch on `dev`'s current stream, its first MM_WS_TICKET_BYTES zero when that launch runs (the C
    ABI's MM_WS_TICKETS_ZEROED contract); the C ABI itself never allocates.

    Eager: one tensor per (device, stream), cleared when it is created and left zero by every launch, grown when a shape needs
    more; consecutive launches of the stream reuse it in stream order.  At most _SPLIT_WS_MAX are kept: dropping a tensor only
    returns its block to the caching allocator's pool of the stream it was allocated on, which hands it to LATER work of that
    stream, so queued launches are not disturbed.

    Under hipGraph capture: a tensor of the capture's own (private pool) with a clearing kernel node for its ticket words in front of the
    launch, on every call.  A captured launch therefore never shares ticket counters with eager work or with another graph --
    whichever stream the graphs are replayed on, in whatever order -- and nothing depends on a clearing that capture recorded
    instead of executing (the first capture used to create, and "zero", the capture stream's workspace)."""
    stream = torch.cuda.current_stream(dev).cuda_stream
    if torch.cuda.is_current_stream_capturing():
        t = torch.empty((max(int(nbytes), _lib.MM_WS_TICKET_BYTES),), dtype=torch.uint8, device=dev)
        with _on_device(dev.index):
            st = _lib.load().mm_matmul_ws_reset(t.data_ptr(), t.numel(), stream)
        if st:
            _lib.check(st, "matmul(workspace)")
        return t
    key = (dev.index, stream)
    t = _SPLIT_WS.get(key)
    if t is None or t.numel() < nbytes:
        size = max(int(nbytes), 8 << 20, 2 * t.numel() if t is not None else 0)
        _SPLIT_WS.pop(key, None)
        t = torch.empty((size,), dtype=torch.uint8, device=dev)
        with _on_device(dev.index):
            st = _lib.load().mm_matmul_ws_reset(t.data_ptr(), t.numel(), stream)
        if st:
            _lib.check(st, "matmul(workspace)")
        _SPLIT_WS[key] = t
        while len(_SPLIT_WS) > _SPLIT_WS_MAX:
            _SPLIT_WS.pop(next(iter(_SPLIT_WS)))
    return t


def matmul(AN, BN, AS, BS, AO, BO, SFAN, SFBN, SFAS, SFBS, SFAO, SFBO, *, bias=None, rounding="reference", out=None,
           split_k=True, out_dtype=torch.bfloat16):
    """bindings.cpp:50-102.  Returns a new [M, N] bf16 tensor.

    Keyword-only extras (not in the reference): `bias` [N] bf16 fused into the epilogue, `rounding` "reference" (bf16 after
    each segment, as the chained reference kernels) or "fused", `out` to write into an existing tensor, `split_k=False`
    to forbid the K-split the library uses for shapes with few output tiles (it needs a scratch tensor; "force" splits
    wherever the shape allows, for tests), `out_dtype=torch.float32` for the unrounded fp32 accumulator (MM_OUT_F32: the partial
    products of a K-sharded tensor-parallel layer; needs rounding="fused" and no bias).

    Shapes are derived exactly as the reference does (bindings.cpp:66-70) and the weight mode
    from `AS.size(1) == BS.size(1) and AO.size(1) == BO.size(1)` (bindings.cpp:74,87).
    """
    lib = _lib.load()
    tensors = (AN, BN, AS, BS, AO, BO, SFAN, SFBN, SFAS, SFBS, SFAO, SFBO)
    dev = AN.device
    index = dev.index
    u8 = torch.uint8
    for t in tensors:
        if not _ok(t, u8, index):
            names = ("AN", "BN", "AS", "BS", "AO", "BO", "SFAN", "SFBN", "SFAS", "SFBS", "SFAO", "SFBO")
            for n, tt in zip(names, tensors):
                _check_tensor(tt, n, u8, dev)
    M, N = AN.size(0), BN.size(0)
    as1, ao1, bs1, bo1 = AS.size(1), AO.size(1), BS.size(1), BO.size(1)
    KN, KS, KO = AN.size(1) * 2, as1 * 4 // 3, ao1
    same = as1 == bs1 and ao1 == bo1
    wmode = _lib.MM_W_MATCH if same else _lib.MM_W_FP4
    if (BN.size(1) != KN // 2 or bs1 != (KS // 4 * 3 if same else KS // 2) or bo1 != (KO if same else KO // 2)
            or BS.size(0) != N or BO.size(0) != N or BN.dim() != 2):
        exp_b = (KN // 2, KS // 4 * 3 if same else KS // 2, KO if same else KO // 2)
        for n, t, w in zip(("BN", "BS", "BO"), (BN, BS, BO), exp_b):
            if t.dim() != 2 or t.size(0) != N or t.size(1) != w:
                raise RuntimeError(f"{n} has shape {tuple(t.shape)}, expected ({N}, {w})")
    if AS.size(0) != M or AO.size(0) != M:
        raise RuntimeError("AS and AO must be [M, bytes]")
    if (SFAN.numel() < _sf_bytes_w(M, KN) or SFAS.numel() < _sf_bytes_w(M, KS) or SFAO.numel() < _sf_bytes_w(M, KO)
            or SFBN.numel() < _sf_bytes_w(N, KN) or SFBS.numel() < _sf_bytes_w(N, KS) or SFBO.numel() < _sf_bytes_w(N, KO)):
        _check_weight_scales((SFAN, SFAS, SFAO), M, KN, KS, KO, ("SFAN", "SFAS", "SFAO"))
        _check_weight_scales((SFBN, SFBS, SFBO), N, KN, KS, KO, ("SFBN", "SFBS", "SFBO"))
    if rounding == "reference":
        flags = _lib.MM_ROUND_PER_SEGMENT
    elif rounding == "fused":
        flags = _lib.MM_ROUND_ONCE
    else:
        raise ValueError("rounding must be 'reference' or 'fused'")
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("out_dtype must be torch.bfloat16 or torch.float32")
    if out_dtype == torch.float32:
        if rounding != "fused" or bias is not None:
            raise ValueError("out_dtype=torch.float32 (fp32 partial sums) needs rounding='fused' and no bias")
        flags |= _lib.MM_OUT_F32
    if bias is not None:
        if not _ok(bias, torch.bfloat16, index):
            _check_tensor(bias, "bias", torch.bfloat16, dev)
        if bias.numel() != N:
            raise RuntimeError("bias must have N elements")
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype, device=dev)
    else:
        if not _ok(out, out_dtype, index):
            _check_tensor(out, "out", out_dtype, dev)
        if out.dim() != 2 or out.size(0) != M or out.size(1) != N:
            raise RuntimeError("out has the wrong shape")
    # the kernels move operands in 16-byte pieces (LDS-DMA, dwordx4 loads): views at odd offsets are rejected, not mis-read
    for t in tensors:
        if t.data_ptr() & 15 and t.numel():
            raise RuntimeError("matmul operands must be 16-byte aligned (got a view at an unaligned offset)")
    if out.data_ptr() & 15:
        raise RuntimeError("out must be 16-byte aligned")
    # shapes with few output tiles split K and need scratch for fp32 partial sums; it comes from torch's caching allocator
    # (stream-ordered, graph-capture safe) because the C ABI never allocates
    ws, ws_bytes = None, 0
    if split_k and M > 32:
        if split_k == "force":
            flags |= _lib.MM_SPLIT_K_ALWAYS
        flags |= _lib.MM_WS_TICKETS_ZEROED
        ws_bytes = lib.mm_matmul_workspace_bytes(M, N, KN, KS, KO, wmode, flags)
        if ws_bytes:
            ws = split_workspace(dev, ws_bytes)
            ws_bytes = ws.numel()
    with _on_device(index):
        st = lib.mm_matmul_ws(_ptr(AN), _ptr(BN), _ptr(AS), _ptr(BS), _ptr(AO), _ptr(BO), _ptr(SFAN), _ptr(SFBN),
                              _ptr(SFAS), _ptr(SFBS), _ptr(SFAO), _ptr(SFBO), M, N, KN, KS, KO, wmode, flags,
                              _ptr(bias) if bias is not None else None, _ptr(out), _ptr(ws) if ws is not None else None,
                              ws_bytes, _stream_ptr(dev))
    if st:
        _lib.check(st, "matmul")
    return out


def interleave_gate_up(gate, up):
    """(BN, BS, BO, SFBN, SFBS, SFBO) of gate_proj and of up_proj -- same shapes, packed with the SAME reorder index and split, fp4
    weights -- as the ONE packed weight of 2 I rows that `gate_up_activate` takes: 128 gate rows alternate with the 128 up rows of the
    same feature indices (one 256-feature GEMM tile then holds everything 128 columns of silu(gate) * up need); the scale tensors,
    whose 128-row tiles are contiguous blocks of (Kseg / 128) * 512 bytes, interleave the same way.  I must be a multiple of 128."""
    n = gate[0].size(0)
    if n % 128 or any(g.shape != u.shape for g, u in zip(gate, up)):
        raise RuntimeError("gate and up must have identical packed shapes and a multiple of 128 output features")
    out = []
    for g, u in zip(gate[:3], up[:3]):
        w = g.size(1)
        out.append(torch.stack((g.reshape(n // 128, 128, w), u.reshape(n // 128, 128, w)), dim=1).reshape(2 * n, w).contiguous())
    for g, u in zip(gate[3:], up[3:]):
        if g.numel() == 0:
            out.append(g.clone())
            continue
        per = g.numel() // (n // 128)
        out.append(torch.stack((g.reshape(n // 128, per), u.reshape(n // 128, per)), dim=1).reshape(-1).contiguous())
    return tuple(out)


def deinterleave_gate_up(packed):
    """inverse of interleave_gate_up: (gate 6-tuple, up 6-tuple), as contiguous copies"""
    n2 = packed[0].size(0)
    n = n2 // 2
    gate, up = [], []
    for t in packed[:3]:
        v = t.reshape(n // 128, 2, 128, t.size(1))
        gate.append(v[:, 0].reshape(n, t.size(1)).contiguous())
        up.append(v[:, 1].reshape(n, t.size(1)).contiguous())
    for t in packed[3:]:
        if t.numel() == 0:
            gate.append(t.clone())
            up.append(t.clone())
            continue
        v = t.reshape(n // 128, 2, -1)
        gate.append(v[:, 0].reshape(-1).contiguous())
        up.append(v[:, 1].reshape(-1).contiguous())
    return tuple(gate), tuple(up)


def gate_up_activate(A, B, DN, DS, DO, *, rounding="reference"):
    """silu(gate_proj(x)) * up_proj(x), quantized for down_proj, as ONE launch for M > 64 (the reference: model/qLlamaLayer.py:377-387
    through HBM; its activate_quantize_x, bindings.cpp:307-334).  A = (AN, AS, AO, SFAN, SFAS, SFAO) = reorder_quantize_x(x, ...);
    B = interleave_gate_up(gate packed, up packed); (DN, DS, DO) = down_proj's split of the I intermediate features in natural
    column order.  Returns (XN, XS, XO, SFXN, SFXS, SFXO), bit-identical to
    `activate_quantize_x(matmul(A, gate), matmul(A, up), DN, DS, DO)`.  Not an export of the reference module."""
    lib = _lib.load()
    dev = A[0].device
    index = dev.index
    u8 = torch.uint8
    for t in (*A, *B):
        if not _ok(t, u8, index):
            _check_tensor(t, "operand", u8, dev)
    M, N2 = A[0].size(0), B[0].size(0)
    KN, KS, KO = A[0].size(1) * 2, A[1].size(1) * 4 // 3, A[2].size(1)
    DN, DS, DO = int(DN), int(DS), int(DO)
    I = N2 // 2
    if N2 % 256 or B[0].size(1) != KN // 2 or B[1].size(1) != KS // 2 or B[2].size(1) != KO // 2 or B[1].size(0) != N2 or B[2].size(0) != N2:
        raise RuntimeError("B must be an interleaved fp4 gate/up weight (interleave_gate_up) matching the activations' split")
    if A[1].size(0) != M or A[2].size(0) != M:
        raise RuntimeError("AS and AO must be [M, bytes]")
    if DN < 0 or DS < 0 or DO < 0 or DN % 128 or DS % 128 or DO % 128 or DN + DS + DO != I:
        _check_split(DN, DS, DO, I, "activate_quantize_x")
    if A[3].numel() < _sf_bytes_w(M, KN) or A[4].numel() < _sf_bytes_w(M, KS) or A[5].numel() < _sf_bytes_w(M, KO):
        _check_weight_scales(A[3:], M, KN, KS, KO, ("SFAN", "SFAS", "SFAO"))
    if B[3].numel() < _sf_bytes_w(N2, KN) or B[4].numel() < _sf_bytes_w(N2, KS) or B[5].numel() < _sf_bytes_w(N2, KO):
        _check_weight_scales(B[3:], N2, KN, KS, KO, ("SFBN", "SFBS", "SFBO"))
    for t in (*A, *B):
        if t.data_ptr() & 15 and t.numel():
            raise RuntimeError("operands must be 16-byte aligned")
    if rounding not in ("reference", "fused"):
        _round_flags(rounding)
    flags = _lib.MM_ROUND_PER_SEGMENT if rounding == "reference" else _lib.MM_ROUND_ONCE
    oN = torch.empty((M, DN // 2), dtype=u8, device=dev)
    oS = torch.empty((M, DS // 4 * 3), dtype=u8, device=dev)
    oO = torch.empty((M, DO), dtype=u8, device=dev)
    sfN = torch.empty((_sf_bytes_x(M, DN),), dtype=u8, device=dev)
    sfS = torch.empty((_sf_bytes_x(M, DS),), dtype=u8, device=dev)
    sfO = torch.empty((_sf_bytes_x(M, DO),), dtype=u8, device=dev)
    ws_bytes = lib.mm_gate_up_activate_workspace_bytes(M, I)
    ws = torch.empty((ws_bytes,), dtype=u8, device=dev) if ws_bytes else None      # stream-ordered scratch from the caching allocator
    with _on_device(index):
        st = lib.mm_gate_up_activate(_ptr(A[0]), _ptr(B[0]), _ptr(A[1]), _ptr(B[1]), _ptr(A[2]), _ptr(B[2]), _ptr(A[3]), _ptr(B[3]),
                                     _ptr(A[4]), _ptr(B[4]), _ptr(A[5]), _ptr(B[5]), M, I, KN, KS, KO, DN, DS, DO, flags,
                                     _ptr(oN), _ptr(oS), _ptr(oO), _ptr(sfN), _ptr(sfS), _ptr(sfO),
                                     _ptr(ws) if ws is not None else None, ws_bytes, _stream_ptr(dev))
    if st:
        _lib.check(st, "gate_up_activate")
    return oN, oS, oO, sfN, sfS, sfO


def reorder_quantize_x_grouped(Xs, reorder_indices, KN, KS, KO):
    """`[reorder_quantize_x(X_g, idx_g, KN, KS, KO) for g]` for row sets that share K and the split (the tokens routed to each MoE
    expert, every expert with its own reorder index; qMixtralLayer.py:507-519), 8 groups per launch, bit-identical to the
    separate calls.  Returns a list of 6-tuples.  Not an export of the reference module."""
    lib = _lib.load()
    if len(Xs) != len(reorder_indices):
        raise ValueError("one reorder index per group")
    if not Xs:
        return []
    KN, KS, KO = int(KN), int(KS), int(KO)
    dev = Xs[0].device
    index = dev.index
    K = Xs[0].size(1)
    if KN < 0 or KS < 0 or KO < 0 or KN % 128 or KS % 128 or KO % 128 or KN + KS + KO != K:
        _check_split(KN, KS, KO, K, "reorder_quantize_x")
    arr = (_lib.MMQuantGroup * len(Xs))()
    res = []
    u8 = torch.uint8
    for g, (X, idx) in enumerate(zip(Xs, reorder_indices)):
        if not (_ok(X, torch.bfloat16, index) and _ok(idx, torch.int16, index)) or X.dim() != 2 or X.size(1) != K or idx.numel() != K:
            _check_tensor(X, f"X[{g}]", torch.bfloat16, dev)
            _check_tensor(idx, f"reorder_index[{g}]", torch.int16, dev)
            raise RuntimeError(f"group {g}: X must be [rows, {K}] and its reorder index must have {K} entries")
        rows = X.size(0)
        out = (torch.empty((rows, KN // 2), dtype=u8, device=dev), torch.empty((rows, KS // 4 * 3), dtype=u8, device=dev),
               torch.empty((rows, KO), dtype=u8, device=dev), torch.empty((_sf_bytes_x(rows, KN),), dtype=u8, device=dev),
               torch.empty((_sf_bytes_x(rows, KS),), dtype=u8, device=dev), torch.empty((_sf_bytes_x(rows, KO),), dtype=u8, device=dev))
        res.append(out)
        e = arr[g]
        e.src_bf16, e.reorder_index = _ptr(X), _ptr(idx)
        e.oN, e.oS, e.oO, e.sfN, e.sfS, e.sfO = (_ptr(t) for t in out)
        e.rows = rows
    with _on_device(index):
        st = lib.mm_reorder_quantize_grouped(arr, len(Xs), K, KN, KS, KO, _lib.MM_QUANT_MIXED, _stream_ptr(dev))
    if st:
        _lib.check(st, "reorder_quantize_x")
    return res


def matmul_grouped(As, Bs, *, biases=None, rounding="reference", outs=None):
    """`[matmul(*interleave(A_g, B_g)) for g]` for groups that share N, the (KN, KS, KO) split and the weight mode -- MoE experts
    (the per-expert loop of qMixtralLayer.py:507-519) -- in as few launches as possible: groups of <= 64 token rows run 8 per
    launch.  As[g] = (AN, AS, AO, SFAN, SFAS, SFAO) as returned by reorder_quantize_x, Bs[g] = (BN, BS, BO, SFBN, SFBS, SFBO).
    Returns the list of [M_g, N] bf16 outputs, bit-identical to the separate calls.  `outs`: one contiguous [M_g, N] bf16 tensor per
    group to write into instead (row slices of one buffer, say); they are returned.  Not an export of the reference module."""
    lib = _lib.load()
    if len(As) != len(Bs) or (biases is not None and len(biases) != len(As)) or (outs is not None and len(outs) != len(As)):
        raise ValueError("As, Bs (and biases, outs) must have one entry per group")
    if not As:
        return []
    dev = As[0][0].device
    index = dev.index
    u8 = torch.uint8
    BN0, BS0, BO0 = Bs[0][0], Bs[0][1], Bs[0][2]
    N = BN0.size(0)
    KN, KS, KO = As[0][0].size(1) * 2, As[0][1].size(1) * 4 // 3, As[0][2].size(1)
    same = As[0][1].size(1) == BS0.size(1) and As[0][2].size(1) == BO0.size(1)
    wmode = _lib.MM_W_MATCH if same else _lib.MM_W_FP4
    wb = (KN // 2, KS // 4 * 3 if same else KS // 2, KO if same else KO // 2)
    if rounding not in ("reference", "fused"):
        _round_flags(rounding)
    flags = _lib.MM_ROUND_PER_SEGMENT if rounding == "reference" else _lib.MM_ROUND_ONCE
    arr = (_lib.MMGroup * len(As))()
    given, outs = outs, []
    for g, (A, B) in enumerate(zip(As, Bs)):
        for t in (*A, *B):
            if not _ok(t, u8, index):
                _check_tensor(t, f"group {g} operand", u8, dev)
        M = A[0].size(0)
        if (A[0].size(1) * 2, A[1].size(1) * 4 // 3, A[2].size(1)) != (KN, KS, KO) or A[1].size(0) != M or A[2].size(0) != M:
            raise RuntimeError(f"group {g}: activation segments do not match the split of group 0")
        if tuple(t.size(0) for t in B[:3]) != (N, N, N) or tuple(t.size(1) for t in B[:3]) != wb:
            raise RuntimeError(f"group {g}: packed weights do not match N / split / weight mode of group 0")
        if (A[3].numel() < _sf_bytes_w(M, KN) or A[4].numel() < _sf_bytes_w(M, KS) or A[5].numel() < _sf_bytes_w(M, KO)
                or B[3].numel() < _sf_bytes_w(N, KN) or B[4].numel() < _sf_bytes_w(N, KS) or B[5].numel() < _sf_bytes_w(N, KO)):
            raise RuntimeError(f"group {g}: a scale tensor is too small")
        bias = biases[g] if biases is not None else None
        if bias is not None and (not _ok(bias, torch.bfloat16, index) or bias.numel() != N):
            raise RuntimeError(f"group {g}: bias must be a bfloat16 tensor with N elements")
        if given is None:
            out = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
        else:
            out = given[g]
            if not _ok(out, torch.bfloat16, index) or tuple(out.shape) != (M, N):
                _check_tensor(out, f"outs[{g}]", torch.bfloat16, dev)
                raise RuntimeError(f"group {g}: outs[{g}] must be [{M}, {N}] bf16")
        outs.append(out)
        e = arr[g]
        e.AN, e.AS, e.AO, e.SFAN, e.SFAS, e.SFAO = (_ptr(t) for t in A)
        e.BN, e.BS, e.BO, e.SFBN, e.SFBS, e.SFBO = (_ptr(t) for t in B)
        e.bias_bf16 = _ptr(bias) if bias is not None else None
        e.D = _ptr(out)
        e.M = M
    with _on_device(index):
        st = lib.mm_matmul_grouped(arr, len(As), N, KN, KS, KO, wmode, flags, _stream_ptr(dev))
    if st:
        _lib.check(st, "matmul_grouped")
    return outs


def _wmode_of(weight_mode):
    if weight_mode not in ("w4", "w"):
        raise ValueError("weight_mode must be 'w4' (fp4 weights, reorder_quantize_w4) or 'w' (matching precision, reorder_quantize_w)")
    return _lib.MM_W_FP4 if weight_mode == "w4" else _lib.MM_W_MATCH


def qlinear_decode_supported(M, N, KN, KS, KO, weight_mode="w4"):
    """0: `qlinear_decode` cannot run this shape (needs 1 <= M <= 8 and the quantized rows in LDS); 1: it can; 2: it can and is
    expected to be faster than reorder_quantize_x + matmul.  `weight_mode`: the packing of the weights the call will get ("w4": the
    production mode; its ring in LDS is the smaller one, so longer K fit: mm_qlinear_decode_supported_w)."""
    return int(_lib.load().mm_qlinear_decode_supported_w(int(M), int(N), int(KN), int(KS), int(KO), _wmode_of(weight_mode)))


def gate_up_activate_decode(X, reorder_index, B, DN, DS, DO, *, rounding="reference"):
    """`gate_up_activate(reorder_quantize_x(X, reorder_index, KN, KS, KO), B, DN, DS, DO)` for decode-sized batches in TWO launches
    instead of three: reorder + quantize + the gate | up GEMM as one launch (`qlinear_decode` on the interleaved weight B), then
    silu(gate) * up + the quantization for down_proj.  X [M, K] bf16 with M <= 8 and `qlinear_decode_supported(M, 2 I, KN, KS, KO)`;
    (KN, KS, KO) are read off B.  Same bytes as the three-launch form.  Not an export of the reference module."""
    return _gate_up_activate_decode(False, X, None, 0.0, reorder_index, B, DN, DS, DO, rounding, True)[1:]


def rmsnorm_gate_up_activate_decode_supported(M, I, KN, KS, KO):
    """0: cannot run; 1: runs; 2: ONE launch with everything inside and expected to be the fastest form of the MLP's first half (M <= 2 on
    a wide layer; mm_rmsnorm_gate_up_activate_decode_supported)"""
    return int(_lib.load().mm_rmsnorm_gate_up_activate_decode_supported(int(M), int(I), int(KN), int(KS), int(KO)))


def gate_up_activate_decode_supported(M, I, KN, KS, KO):
    """the same for `gate_up_activate_decode` (no norm)"""
    return int(_lib.load().mm_gate_up_activate_decode_supported(int(M), int(I), int(KN), int(KS), int(KO)))


def _residual_operands(X, residual, out_sum, index):
    """the residual and the tensor that receives X + residual, checked (the library itself refuses an out_sum that overlaps either input)"""
    if not _ok(residual, torch.bfloat16, index) or tuple(residual.shape) != tuple(X.shape):
        _check_tensor(residual, "residual", torch.bfloat16, X.device)
        raise RuntimeError("residual must have X's shape")
    if out_sum is None:
        out_sum = torch.empty_like(X)
    elif not _ok(out_sum, torch.bfloat16, index) or tuple(out_sum.shape) != tuple(X.shape):
        _check_tensor(out_sum, "out_sum", torch.bfloat16, X.device)
        raise RuntimeError("out_sum must have X's shape")
    return out_sum


def add_rmsnorm_gate_up_activate_decode(X, residual, norm_weight, eps, reorder_index, B, DN, DS, DO, *, rounding="reference", integer_round=True,
                                        out_sum=None):
    """`rmsnorm_gate_up_activate_decode` on s = X + residual (torch's bf16 add), the add inside the launch: returns (s, down_proj's six
    operands).  Bit-identical to `add_rmsnorm_quantize_x` -> `gate_up_activate`; supported where the plain form is."""
    res = _gate_up_activate_decode(True, X, norm_weight, eps, reorder_index, B, DN, DS, DO, rounding, integer_round, residual, out_sum)
    return res if residual is not None else res[1:]      # (no residual: the plain norm form and its six operands, as ever)


def rmsnorm_gate_up_activate_decode(X, norm_weight, eps, reorder_index, B, DN, DS, DO, *, rounding="reference", integer_round=True):
    """`gate_up_activate(rmsnorm_quantize_x(X, norm_weight, eps, reorder_index, KN, KS, KO), B, DN, DS, DO)` for decode-sized batches: the
    post-attention RMSNorm, the quantization of x, the gate | up GEMM on the interleaved weight B, silu(gate) * up and the quantization for
    down_proj -- ONE launch on a wide layer at M <= 4, two otherwise (`rmsnorm_gate_up_activate_decode_supported(...) == 2`: where it is the
    fastest form).  Returns
    down_proj's activation operands (oN, oS, oO, sfN, sfS, sfO): `matmul` them with the packed down_proj weight.  Same bytes as the
    three-op form.  Not an export of the reference module."""
    return _gate_up_activate_decode(True, X, norm_weight, eps, reorder_index, B, DN, DS, DO, rounding, integer_round)[1:]


def _gate_up_activate_decode(norm, X, norm_weight, eps, reorder_index, B, DN, DS, DO, rounding, integer_round, residual=None, out_sum=None):
    """shared body of gate_up_activate_decode (norm False), rmsnorm_gate_up_activate_decode and add_rmsnorm_gate_up_activate_decode
    (residual given): (out_sum or None, oN, oS, oO, sfN, sfS, sfO).  `norm` says which form runs, never norm_weight: None there is an error"""
    lib = _lib.load()
    dev = X.device
    index = dev.index
    if not (X.is_cuda and _ok(X, torch.bfloat16, index) and _ok(reorder_index, torch.int16, index) and (not norm or _ok(norm_weight, torch.bfloat16, index))):
        _check_tensor(X, "X", torch.bfloat16)
        if norm:
            _check_tensor(norm_weight, "norm_weight", torch.bfloat16, dev)
        _check_tensor(reorder_index, "reorder_index", torch.int16, dev)
    if residual is not None:
        out_sum = _residual_operands(X, residual, out_sum, index)
    for t in B:
        if not _ok(t, torch.uint8, index):
            _check_tensor(t, "operand", torch.uint8, dev)
    M, K = X.shape
    N2 = B[0].size(0)
    KN, KS, KO = B[0].size(1) * 2, B[1].size(1) * 2, B[2].size(1) * 2
    I = N2 // 2
    DN, DS, DO = int(DN), int(DS), int(DO)
    if N2 % 256 or K != KN + KS + KO or reorder_index.numel() != K or (norm and norm_weight.numel() != K) or B[1].size(0) != N2 or B[2].size(0) != N2:
        raise RuntimeError("B must be an interleaved fp4 gate/up weight (interleave_gate_up) whose split adds up to X's columns")
    if DN < 0 or DS < 0 or DO < 0 or DN % 128 or DS % 128 or DO % 128 or DN + DS + DO != I:
        _check_split(DN, DS, DO, I, "activate_quantize_x")
    if B[3].numel() < _sf_bytes_w(N2, KN) or B[4].numel() < _sf_bytes_w(N2, KS) or B[5].numel() < _sf_bytes_w(N2, KO):
        _check_weight_scales(B[3:], N2, KN, KS, KO, ("SFBN", "SFBS", "SFBO"))
    if rounding not in ("reference", "fused"):
        _round_flags(rounding)
    flags = _lib.MM_ROUND_PER_SEGMENT if rounding == "reference" else _lib.MM_ROUND_ONCE
    if not integer_round:
        flags |= _lib.MM_NORM_NO_INTEGER_ROUND
    u8 = torch.uint8
    oN = torch.empty((M, DN // 2), dtype=u8, device=dev)
    oS = torch.empty((M, DS // 4 * 3), dtype=u8, device=dev)
    oO = torch.empty((M, DO), dtype=u8, device=dev)
    sfN = torch.empty((_sf_bytes_x(M, DN),), dtype=u8, device=dev)
    sfS = torch.empty((_sf_bytes_x(M, DS),), dtype=u8, device=dev)
    sfO = torch.empty((_sf_bytes_x(M, DO),), dtype=u8, device=dev)
    ws = torch.empty((M * N2 * 2,), dtype=u8, device=dev)      # (scratch of the two-launch form; stream-ordered, from the caching allocator)
    tail = (_ptr(reorder_index), _ptr(B[0]), _ptr(B[1]), _ptr(B[2]), _ptr(B[3]), _ptr(B[4]), _ptr(B[5]), M, I, KN, KS, KO, DN, DS, DO, flags, _ptr(oN),
            _ptr(oS), _ptr(oO), _ptr(sfN), _ptr(sfS), _ptr(sfO), _ptr(ws), ws.numel(), _stream_ptr(dev))
    with _on_device(index):
        if not norm:
            st, what = lib.mm_gate_up_activate_decode(_ptr(X), *tail), "gate_up_activate_decode"
        elif residual is None:
            st, what = lib.mm_rmsnorm_gate_up_activate_decode(_ptr(X), _ptr(norm_weight), float(eps), *tail), "rmsnorm_gate_up_activate_decode"
        else:
            st, what = lib.mm_add_rmsnorm_gate_up_activate_decode(_ptr(X), _ptr(residual), _ptr(out_sum), _ptr(norm_weight), float(eps), *tail), \
                "add_rmsnorm_gate_up_activate_decode"
    if st:
        _lib.check(st, what)
    return out_sum, oN, oS, oO, sfN, sfS, sfO


def down_activate_decode_supported(M, N, DN, DS, DO, weight_mode="w4"):
    """0: cannot run; 1: runs; 2: runs and is expected to beat activate_quantize_x + matmul (mm_down_activate_decode_supported_w)"""
    return int(_lib.load().mm_down_activate_decode_supported_w(int(M), int(N), int(DN), int(DS), int(DO), _wmode_of(weight_mode)))


def down_activate_decode(GU, B, DN, DS, DO, *, bias=None, rounding="reference"):
    """down_proj(act_fn(gate) * up) for decode-sized batches in ONE launch: GU [M, 2 I] bf16 holds 128 gate columns alternating with the
    128 up columns of the same indices (what `qlinear_decode` on an `interleave_gate_up` weight returns); B = down_proj packed with
    `downproj_quantize_w4` / `_w`; (DN, DS, DO) = its split of the I intermediate features.  Bit-identical to
    `matmul(activate_quantize_x(gate, up, DN, DS, DO), B)`.  M <= 4.  Not an export of the reference module."""
    lib = _lib.load()
    dev = GU.device
    index = dev.index
    if not (GU.is_cuda and _ok(GU, torch.bfloat16, index)):
        _check_tensor(GU, "GU", torch.bfloat16)
    for t in B:
        if not _ok(t, torch.uint8, index):
            _check_tensor(t, "operand", torch.uint8, dev)
    DN, DS, DO = int(DN), int(DS), int(DO)
    M, I2 = GU.shape
    I = DN + DS + DO
    N = B[0].size(0)
    if I2 != 2 * I or I % 128 or DN % 128 or DS % 128 or DO % 128:
        _lib.check(_lib.MM_ERR_BAD_SPLIT, "activate_quantize_x")
    same = B[1].size(1) == DS // 4 * 3 and B[2].size(1) == DO
    if B[0].size(1) != DN // 2 or not (same or (B[1].size(1) == DS // 2 and B[2].size(1) == DO // 2)) or B[1].size(0) != N or B[2].size(0) != N:
        _weight_mode(B, N, DN, DS, DO, "(DN, DS, DO)")
    wmode = _lib.MM_W_MATCH if same else _lib.MM_W_FP4
    if B[3].numel() < _sf_bytes_w(N, DN) or B[4].numel() < _sf_bytes_w(N, DS) or B[5].numel() < _sf_bytes_w(N, DO):
        _check_weight_scales(B[3:], N, DN, DS, DO)
    if rounding not in ("reference", "fused"):
        _round_flags(rounding)
    flags = _lib.MM_ROUND_PER_SEGMENT if rounding == "reference" else _lib.MM_ROUND_ONCE
    if bias is not None and (not _ok(bias, torch.bfloat16, index) or bias.numel() != N):
        _check_tensor(bias, "bias", torch.bfloat16, dev)
        raise RuntimeError("bias must have N elements")
    out = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
    with _on_device(index):
        st = lib.mm_down_activate_decode(_ptr(GU), _ptr(B[0]), _ptr(B[1]), _ptr(B[2]), _ptr(B[3]), _ptr(B[4]), _ptr(B[5]), M, N, DN, DS, DO, wmode,
                                         flags, _ptr(bias) if bias is not None else None, _ptr(out), _stream_ptr(dev))
    if st:
        _lib.check(st, "down_activate_decode")
    return out


def qlinear_decode(X, reorder_index, BN, BS, BO, SFBN, SFBS, SFBO, KN, KS, KO, *, bias=None, rounding="reference", out=None):
    """reorder_quantize_x + matmul (+ bias) of `QLinearLayer.forward` (qLinearLayer.py:58-74) as ONE launch for M <= 8 rows.

    Not an export of the reference module: it is what the reference's forward computes, fused for decode, and bit-identical
    to the two-op path.  X [M, K] bf16; B / SFB are the layer's packed weights; returns [M, N] bf16.
    """
    return _qlinear_decode(False, X, None, 0.0, reorder_index, BN, BS, BO, SFBN, SFBS, SFBO, KN, KS, KO, bias, rounding, True, out)[1]


def rmsnorm_qlinear_decode_supported(M, N, KN, KS, KO, weight_mode="w4"):
    """0 / 1 / 2 as qlinear_decode_supported, for the launch with the RMSNorm inside (K <= 8192)"""
    return int(_lib.load().mm_rmsnorm_qlinear_decode_supported_w(int(M), int(N), int(KN), int(KS), int(KO), _wmode_of(weight_mode)))


def add_rmsnorm_qlinear_decode(X, residual, norm_weight, eps, reorder_index, BN, BS, BO, SFBN, SFBS, SFBO, KN, KS, KO, *, bias=None,
                               rounding="reference", integer_round=True, out=None, out_sum=None):
    """`rmsnorm_qlinear_decode` on s = X + residual (torch's bf16 add), the add inside the launch: returns (s, D).  Bit-identical to
    `add_rmsnorm_quantize_x` followed by `matmul`; supported where the plain form is (`rmsnorm_qlinear_decode_supported`)."""
    res = _qlinear_decode(True, X, norm_weight, eps, reorder_index, BN, BS, BO, SFBN, SFBS, SFBO, KN, KS, KO, bias, rounding, integer_round, out, residual,
                          out_sum)
    return res if residual is not None else res[1]      # (no residual: the plain norm form and its one tensor, as ever)


def rmsnorm_qlinear_decode(X, norm_weight, eps, reorder_index, BN, BS, BO, SFBN, SFBS, SFBO, KN, KS, KO, *, bias=None, rounding="reference",
                           integer_round=True, out=None):
    """rmsnorm_quantize_x + matmul (+ bias) as ONE launch for M <= 8 rows: what a decoder layer of the reference runs in front of
    q/k/v and gate/up (qLlamaLayer.py: input_layernorm / post_attention_layernorm fused into the quantizer, rmsnorm.cu:95-352, then
    qLinearLayer.py:58-74).  Bit-identical to `rmsnorm_quantize_x` followed by `matmul`.  X [M, K] bf16, norm_weight [K] bf16."""
    return _qlinear_decode(True, X, norm_weight, eps, reorder_index, BN, BS, BO, SFBN, SFBS, SFBO, KN, KS, KO, bias, rounding, integer_round, out)[1]


def _qlinear_decode(norm, X, norm_weight, eps, reorder_index, BN, BS, BO, SFBN, SFBS, SFBO, KN, KS, KO, bias, rounding, integer_round, out,
                    residual=None, out_sum=None):
    """shared body of qlinear_decode (norm False), rmsnorm_qlinear_decode and add_rmsnorm_qlinear_decode (residual given):
    (out_sum or None, out).  `norm` says which form runs, never norm_weight: None there is an error"""
    lib = _lib.load()
    dev = X.device
    index = dev.index
    if residual is not None:
        out_sum = _residual_operands(X, residual, out_sum, index)
    if not (X.is_cuda and _ok(X, torch.bfloat16, index) and _ok(reorder_index, torch.int16, index) and (not norm or _ok(norm_weight, torch.bfloat16, index))):
        _check_tensor(X, "X", torch.bfloat16)
        if norm:
            _check_tensor(norm_weight, "norm_weight", torch.bfloat16, dev)
        _check_tensor(reorder_index, "reorder_index", torch.int16, dev)
    for n, t in (("BN", BN), ("BS", BS), ("BO", BO), ("SFBN", SFBN), ("SFBS", SFBS), ("SFBO", SFBO)):
        if not _ok(t, torch.uint8, index):
            _check_tensor(t, n, torch.uint8, dev)
    KN, KS, KO = int(KN), int(KS), int(KO)
    M, K = X.shape
    N = BN.size(0)
    if K != KN + KS + KO or reorder_index.numel() != K or (norm and norm_weight.numel() != K):
        _lib.check(_lib.MM_ERR_BAD_SPLIT, "rmsnorm_quantize_x" if norm else "reorder_quantize_x")
    # (hot-path rule, here as in every wrapper: the tests inline, the helpers -- which raise -- only once one of them failed)
    same = BS.size(1) == KS // 4 * 3 and BO.size(1) == KO
    if BN.size(1) != KN // 2 or not (same or (BS.size(1) == KS // 2 and BO.size(1) == KO // 2)) or BS.size(0) != N or BO.size(0) != N:
        _weight_mode((BN, BS, BO), N, KN, KS, KO)
    wmode = _lib.MM_W_MATCH if same else _lib.MM_W_FP4
    if SFBN.numel() < _sf_bytes_w(N, KN) or SFBS.numel() < _sf_bytes_w(N, KS) or SFBO.numel() < _sf_bytes_w(N, KO):
        _check_weight_scales((SFBN, SFBS, SFBO), N, KN, KS, KO)
    if rounding not in ("reference", "fused"):
        _round_flags(rounding)
    flags = (_lib.MM_ROUND_PER_SEGMENT if rounding == "reference" else _lib.MM_ROUND_ONCE) | (0 if integer_round else _lib.MM_NORM_NO_INTEGER_ROUND)
    if bias is not None and (not _ok(bias, torch.bfloat16, index) or bias.numel() != N):
        _check_tensor(bias, "bias", torch.bfloat16, dev)
        raise RuntimeError("bias must have N elements")
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
    tail = (_ptr(reorder_index), _ptr(BN), _ptr(BS), _ptr(BO), _ptr(SFBN), _ptr(SFBS), _ptr(SFBO), M, N, KN, KS, KO, wmode, flags,
            _ptr(bias) if bias is not None else None, _ptr(out), _stream_ptr(dev))
    with _on_device(index):
        if not norm:
            st, what = lib.mm_qlinear_decode(_ptr(X), *tail), "qlinear_decode"
        elif residual is None:
            st, what = lib.mm_rmsnorm_qlinear_decode(_ptr(X), _ptr(norm_weight), float(eps), *tail), "rmsnorm_qlinear_decode"
        else:
            st, what = lib.mm_add_rmsnorm_qlinear_decode(_ptr(X), _ptr(residual), _ptr(out_sum), _ptr(norm_weight), float(eps), *tail), \
                "add_rmsnorm_qlinear_decode"
    if st:
        _lib.check(st, what)
    return out_sum, out


def _direct(src_a, src_b, KN, KS, KO, mode, what):
    """shared body of activate_quantize_x / downproj_quantize_w / downproj_quantize_w4 (bindings.cpp:307-387)."""
    lib = _lib.load()
    srcs = (src_a,) if src_b is None else (src_a, src_b)
    for t in srcs:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and _ok(t, torch.bfloat16, src_a.get_device())):
            _check_tensor(t, "input", torch.bfloat16, src_a.device if isinstance(src_a, torch.Tensor) and src_a.is_cuda else None)
    KN, KS, KO = int(KN), int(KS), int(KO)
    if src_a.dim() != 2 or (src_b is not None and tuple(src_b.shape) != tuple(src_a.shape)):
        raise RuntimeError("inputs must be 2-D [rows, K] of equal shape")
    rows, K = src_a.shape
    if KN < 0 or KS < 0 or KO < 0 or KN % 128 or KS % 128 or KO % 128 or KN + KS + KO != K:
        _check_split(KN, KS, KO, K, what)
    dev = src_a.device
    w4 = mode == "w4"
    u8 = torch.uint8
    oN = torch.empty((rows, KN // 2), dtype=u8, device=dev)
    oS = torch.empty((rows, KS // 2 if w4 else KS // 4 * 3), dtype=u8, device=dev)
    oO = torch.empty((rows, KO // 2 if w4 else KO), dtype=u8, device=dev)
    sfN = torch.empty((_sf_bytes_x(rows, KN),), dtype=u8, device=dev)
    sfS = torch.empty((_sf_bytes_x(rows, KS),), dtype=u8, device=dev)
    sfO = torch.empty((_sf_bytes_x(rows, KO),), dtype=u8, device=dev)
    with _on_device(dev.index):
        if src_b is not None:
            st = lib.mm_activate_quantize(_ptr(src_a), _ptr(src_b), rows, KN, KS, KO, _ptr(oN), _ptr(oS), _ptr(oO), _ptr(sfN),
                                          _ptr(sfS), _ptr(sfO), _stream_ptr(dev))
        else:
            st = lib.mm_downproj_quantize(_ptr(src_a), rows, KN, KS, KO, _lib.MM_QUANT_W4 if w4 else _lib.MM_QUANT_MIXED,
                                          _ptr(oN), _ptr(oS), _ptr(oO), _ptr(sfN), _ptr(sfS), _ptr(sfO), _stream_ptr(dev))
    if st:
        _lib.check(st, what)
    return oN, oS, oO, sfN, sfS, sfO


def activate_quantize_x(A, B, KN, KS, KO):
    """bindings.cpp:307-335.  silu(A) * B, natural column order -> (XN, XS, XO, SFXN, SFXS, SFXO)."""
    return _direct(A, B, KN, KS, KO, "x", "activate_quantize_x")


def downproj_quantize_w(W, KN, KS, KO):
    """bindings.cpp:336-362.  W [N,K] in natural column order -> fp4 | fp6 | fp8 segments."""
    return _direct(W, None, KN, KS, KO, "w", "downproj_quantize_w")


def downproj_quantize_w4(W, KN, KS, KO):
    """bindings.cpp:363-387.  W [N,K] in natural column order -> three fp4 segments."""
    return _direct(W, None, KN, KS, KO, "w4", "downproj_quantize_w4")


def _not_on_path(name):
    def f(*a, **k):
        raise NotImplementedError(f"mixedgemm.{name} is outside the MX hot path built here (SURVEY.md section 8f)")
    f.__name__ = name
    return f


def rmsnorm_quantize_x(X, W, eps, reorder_index, KN, KS, KO, *, integer_round=True):
    """bindings.cpp:257-303 / rmsnorm.cu:95-312.  RMSNorm(X; W, eps) -> reorder -> mixed quantize, one kernel.

    X [M,K] bf16, W [K] bf16 norm weight -> (XN [M,KN/2], XS [M,3KS/4], XO [M,KO], SFXN, SFXS, SFXO), the tuple
    `QLinearLayer.forward` accepts in place of a tensor, so q/k/v (or gate/up) share one quantization.
    `integer_round=True` (default) reproduces the reference, which rounds the scaled value to an integer before the element
    conversion (rmsnorm.cu:262-267); `False` drops that step.
    """
    return _rmsnorm_quantize_x(False, X, W, eps, reorder_index, KN, KS, KO, integer_round)[1:]


def add_rmsnorm_quantize_x(x, residual, weight, eps, reorder_index, KN, KS, KO, out_sum=None, *, integer_round=True):
    """The residual add of a decoder layer fused into `rmsnorm_quantize_x`: s = x + residual (torch's bf16 add, bit for bit), then
    RMSNorm(s; weight, eps) -> reorder -> mixed quantize, one kernel that reads x and residual once and writes s once.

    x, residual [M, K] bf16 -> (s, XN, XS, XO, SFXN, SFXS, SFXO): s [M, K] bf16 is the new residual stream, the rest is byte for byte
    `rmsnorm_quantize_x(s, weight, eps, reorder_index, KN, KS, KO)`.  `out_sum`: a [M, K] bf16 tensor to receive s; it must not
    overlap x or residual (the library refuses an overlap).  Not an export of the reference module: its layers add in torch
    (model/qLlamaLayer.py:127-148)."""
    return _rmsnorm_quantize_x(True, x, weight, eps, reorder_index, KN, KS, KO, integer_round, residual, out_sum)


def _rmsnorm_quantize_x(add, X, W, eps, reorder_index, KN, KS, KO, integer_round, residual=None, out_sum=None):
    """shared body of rmsnorm_quantize_x and add_rmsnorm_quantize_x (add True: a residual of None is an error; its errors call the operands x / weight):
    (out_sum or None, oN, oS, oO, sfN, sfS, sfO)"""
    lib = _lib.load()
    if not (isinstance(X, torch.Tensor) and X.is_cuda and (not add or isinstance(residual, torch.Tensor)) and isinstance(W, torch.Tensor)
            and isinstance(reorder_index, torch.Tensor) and _ok(X, torch.bfloat16, X.get_device()) and (not add or _ok(residual, torch.bfloat16, X.get_device()))
            and _ok(W, torch.bfloat16, X.get_device()) and _ok(reorder_index, torch.int16, X.get_device())):
        _check_tensor(X, "x" if add else "X", torch.bfloat16)
        if add:
            _check_tensor(residual, "residual", torch.bfloat16, X.device)
        _check_tensor(W, "weight" if add else "W", torch.bfloat16, X.device)
        _check_tensor(reorder_index, "reorder_index", torch.int16, X.device)
    if X.dim() != 2 or (add and tuple(residual.shape) != tuple(X.shape)):
        raise RuntimeError("x and residual must be 2-D [rows, K] of equal shape" if add else "X must be 2-D [rows, K]")
    KN, KS, KO = int(KN), int(KS), int(KO)
    rows, K = X.shape
    if reorder_index.numel() != K or W.numel() != K:
        _lib.check(_lib.MM_ERR_BAD_SPLIT, "rmsnorm_bf16_mixed")    # bindings.cpp:298 "Value error in run_rmsnorm_bf16_mixed"
    if KN < 0 or KS < 0 or KO < 0 or KN % 128 or KS % 128 or KO % 128 or KN + KS + KO != K:
        _check_split(KN, KS, KO, K, "rmsnorm_bf16_mixed")
    dev = X.device
    if add and out_sum is None:
        out_sum = torch.empty((rows, K), dtype=torch.bfloat16, device=dev)
    elif add and (not _ok(out_sum, torch.bfloat16, X.get_device()) or tuple(out_sum.shape) != (rows, K)):
        _check_tensor(out_sum, "out_sum", torch.bfloat16, dev)
        raise RuntimeError("out_sum must be [rows, K]")
    u8 = torch.uint8
    oN = torch.empty((rows, KN // 2), dtype=u8, device=dev)
    oS = torch.empty((rows, KS // 4 * 3), dtype=u8, device=dev)
    oO = torch.empty((rows, KO), dtype=u8, device=dev)
    sfN = torch.empty((_sf_bytes_x(rows, KN),), dtype=u8, device=dev)
    sfS = torch.empty((_sf_bytes_x(rows, KS),), dtype=u8, device=dev)
    sfO = torch.empty((_sf_bytes_x(rows, KO),), dtype=u8, device=dev)
    tail = (float(eps), rows, K, _ptr(reorder_index), KN, KS, KO, _lib.MM_RMS_REFERENCE if integer_round else _lib.MM_RMS_NO_INTEGER_ROUND,
            _ptr(oN), _ptr(oS), _ptr(oO), _ptr(sfN), _ptr(sfS), _ptr(sfO), _stream_ptr(dev))
    with _on_device(dev.index):
        if add:
            st = lib.mm_add_rmsnorm_quantize(_ptr(X), _ptr(residual), _ptr(out_sum), _ptr(W), *tail)
        else:
            st = lib.mm_rmsnorm_quantize(_ptr(X), _ptr(W), *tail)
    if st:
        _lib.check(st, "add_rmsnorm_quantize_x" if add else "rmsnorm_bf16_mixed")
    return out_sum, oN, oS, oO, sfN, sfS, sfO


for _n in ("batch_decode_i4", "batch_decode_f16", "init_kv_i4", "init_kv_f16", "append_kv_i4", "append_kv_f16"):
    globals()[_n] = _not_on_path(_n)


# ---- paged KV cache (include/micromix_hip.h, mm_kv_append / mm_paged_decode; micromix_amd/kvcache.py is the small cache object) ----

def _kv_bytes(kv_data):
    """an fp8 cache held as torch.float8_e4m3fn, seen as the uint8 tensor the ops take: the same bytes, OCP e4m3fn codes"""
    return kv_data.view(torch.uint8) if isinstance(kv_data, torch.Tensor) and kv_data.dtype is torch.float8_e4m3fn else kv_data


def _kv_geometry(kv_data, kv_param, index):
    """(dtype code, max_pages, L, Hkv, P, kv_data as the C ABI takes it) of a cache, recognised by its shape; int4: uint8
    [max_pages, L, 2, Hkv, P, 64] + fp16 params [..., P, 2]; fp8: uint8 (or torch.float8_e4m3fn, viewed as uint8) [max_pages, L, 2, Hkv,
    P, 128] + the same fp16 params; bf16: bf16 [max_pages, L, 2, Hkv, P, 128] and kv_param None."""
    if kv_param is None:
        if not _ok(kv_data, torch.bfloat16, index):
            _check_tensor(kv_data, "kv_data", torch.bfloat16)
            raise RuntimeError(f"kv_data must be on cuda:{index}")
        if kv_data.dim() != 6 or kv_data.size(2) != 2 or kv_data.size(5) != 128:
            raise RuntimeError("bf16 kv_data (kv_param None) must be [max_pages, L, 2, Hkv, P, 128]; an int4 cache ([..., 64] uint8) and an "
                               "fp8 cache ([..., 128] uint8 / float8_e4m3fn) need their fp16 kv_param")
        kind = _lib.MM_KV_BF16
    else:
        kv_data = _kv_bytes(kv_data)
        if not (_ok(kv_data, torch.uint8, index) and _ok(kv_param, torch.float16, index)):
            _check_tensor(kv_data, "kv_data", torch.uint8)
            _check_tensor(kv_param, "kv_param", torch.float16, kv_data.device)
            raise RuntimeError(f"kv_data / kv_param must be on cuda:{index}")
        if kv_data.dim() != 6 or kv_data.size(2) != 2 or kv_data.size(5) not in (64, 128):
            raise RuntimeError("kv_data with a kv_param must be [max_pages, L, 2, Hkv, P, 64] uint8 (int4) or [max_pages, L, 2, Hkv, P, 128] "
                               "uint8 / float8_e4m3fn (fp8); a bf16 cache [max_pages, L, 2, Hkv, P, 128] takes kv_param None")
        if tuple(kv_param.shape) != tuple(kv_data.shape[:5]) + (2,):
            raise RuntimeError("kv_param must be [max_pages, L, 2, Hkv, P, 2] fp16, matching kv_data")
        kind = _lib.MM_KV_INT4 if kv_data.size(5) == 64 else _lib.MM_KV_FP8_E4M3
    max_pages, L, _, Hkv, P, _ = kv_data.shape
    return kind, max_pages, L, Hkv, P, kv_data


def _page_table(kv_indptr, kv_indices, last_page_len, dev):
    for n, t in (("kv_indptr", kv_indptr), ("kv_indices", kv_indices), ("last_page_len", last_page_len)):
        if not _ok(t, torch.int32, dev.index):
            _check_tensor(t, n, torch.int32, dev)
    B = last_page_len.numel()
    if kv_indptr.numel() != B + 1:
        raise RuntimeError("kv_indptr must have B + 1 entries (B = last_page_len.numel())")
    return B


def _kv_args(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, layer_idx, q=None):
    """The common checks of the four cache ops: (device, B, Hkv, the C arguments kv_data .. batch that every entry point takes in this
    order).  The device is q's (bf16, contiguous); an append has no q and takes the cache's."""
    if kv_param is not None:
        kv_data = _kv_bytes(kv_data)
    if q is None:
        if not (isinstance(kv_data, torch.Tensor) and kv_data.is_cuda):
            _check_tensor(kv_data, "kv_data", torch.uint8 if kv_param is not None else torch.bfloat16)
        dev = kv_data.device
    else:
        if not (isinstance(q, torch.Tensor) and q.is_cuda and _ok(q, torch.bfloat16, q.get_device())):
            _check_tensor(q, "q", torch.bfloat16)
        dev = q.device
    kind, max_pages, L, Hkv, P, kv_data = _kv_geometry(kv_data, kv_param, dev.index)
    B = _page_table(kv_indptr, kv_indices, last_page_len, dev)
    layer_idx = int(layer_idx)
    if not 0 <= layer_idx < L:
        raise RuntimeError(f"layer_idx {layer_idx} outside the cache's {L} layers")
    return dev, B, Hkv, (_ptr(kv_data), _ptr(kv_param) if kv_param is not None else None, kind, max_pages, L, layer_idx, Hkv, P, 128,
                         _ptr(kv_indptr), _ptr(kv_indices), _ptr(last_page_len), B)


def _kv_workspace(workspace, need, dev):
    """(the split-KV scratch, which the caller holds across the launch, its two C arguments): allocated when `need` bytes are wanted and
    none was passed"""
    if not need:
        return None, (None, 0)
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
    if (not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or workspace.device != dev
            or not workspace.is_contiguous() or workspace.numel() * workspace.element_size() < need):
        raise RuntimeError(f"workspace must be a contiguous device tensor of at least {need} bytes on {dev}")
    return workspace, (_ptr(workspace), workspace.numel() * workspace.element_size())


def _sm_scale(sm_scale):
    scale = float(sm_scale) if sm_scale is not None else 128 ** -0.5
    if not scale > 0:
        raise ValueError("sm_scale must be positive")
    return scale


def kv_append(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, k, v, append_indptr, layer_idx):
    """Write T new tokens' K and V (bf16 [T, Hkv, 128]) into layer `layer_idx` of a paged cache, in place.

    Not an export of the reference module (its append_kv_i4 / _f16 take K/V already quantized and one head count).  The page table
    (kv_indptr [B + 1], kv_indices, last_page_len [B], int32) already counts the new tokens; append_indptr [B + 1] splits the T tokens
    among the sequences, each sequence's go to its last positions.  kv_param None: bf16 cache (a copy); otherwise int4 codes + fp16
    (scale, zero) by the rule of quantize_int_group(x, 4, 128), or -- kv_data [..., 128] uint8 / float8_e4m3fn -- e4m3 codes with a
    power-of-two scale per row and zero = 0 (include/micromix_hip.h, MM_KV_FP8_E4M3).  Runs on the current stream, capture-safe.
    """
    lib = _lib.load()
    dev, B, Hkv, kv_args = _kv_args(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, layer_idx)
    if not _ok(append_indptr, torch.int32, dev.index):
        _check_tensor(append_indptr, "append_indptr", torch.int32, dev)
    for n, t in (("k", k), ("v", v)):
        if not _ok(t, torch.bfloat16, dev.index):
            _check_tensor(t, n, torch.bfloat16, dev)
    if k.dim() != 3 or k.shape != v.shape or k.size(1) != Hkv or k.size(2) != 128:
        raise RuntimeError(f"k and v must both be [T, {Hkv}, 128] bf16")
    if append_indptr.numel() != B + 1:
        raise RuntimeError("append_indptr must have B + 1 entries")
    with _on_device(dev.index):
        st = lib.mm_kv_append(*kv_args, _ptr(k), _ptr(v), _ptr(append_indptr), k.size(0), _stream_ptr(dev))
    if st:
        _lib.check(st, "kv_append")


def kv_copy_pages(kv_data, kv_param, src_pages, dst_pages, rows=None):
    """Copy token rows [0, rows[i]) of page src_pages[i] to page dst_pages[i] of a paged cache, for every layer, K and V, every head, in
    place; returns None.  rows None: whole pages.  Bytes only (codes and, for int4 / fp8, the fp16 params): no dequantization.

    src_pages, dst_pages, rows: int32 device tensors of one length.  A pair whose page index lies outside the cache, with src == dst or
    with rows <= 0 is skipped; rows above the page size count as the page size.  The destination pages must be pairwise distinct and
    none of them a source of the same call (include/micromix_hip.h, mm_kv_copy_pages).  What PagedKVCache.extend calls before a sequence
    writes into a partly filled page it shares.  Runs on the current stream, capture-safe."""
    lib = _lib.load()
    if kv_param is not None:
        kv_data = _kv_bytes(kv_data)
    if not (isinstance(kv_data, torch.Tensor) and kv_data.is_cuda):
        _check_tensor(kv_data, "kv_data", torch.uint8 if kv_param is not None else torch.bfloat16)
    dev = kv_data.device
    kind, max_pages, L, Hkv, P, kv_data = _kv_geometry(kv_data, kv_param, dev.index)
    index = [("src_pages", src_pages), ("dst_pages", dst_pages)] + ([("rows", rows)] if rows is not None else [])
    for n, t in index:
        if not _ok(t, torch.int32, dev.index):
            _check_tensor(t, n, torch.int32, dev)
        if t.dim() != 1 or t.numel() != src_pages.numel():
            raise RuntimeError("src_pages, dst_pages and rows must be one-dimensional and of one length")
    with _on_device(dev.index):
        st = lib.mm_kv_copy_pages(_ptr(kv_data), _ptr(kv_param) if kv_param is not None else None, kind, max_pages, L, Hkv, P, 128,
                                  _ptr(src_pages), _ptr(dst_pages), _ptr(rows) if rows is not None else None, src_pages.numel(),
                                  _stream_ptr(dev))
    if st:
        _lib.check(st, "kv_copy_pages")


def _tree_lib():
    lib = _lib.load()
    if not hasattr(lib, "mm_paged_prefill_tree"):
        raise _lib.MicroMixLibraryError("libmicromix_hip.so has no mm_paged_prefill_tree / mm_kv_move_rows: it was built before tree-masked "
                                        "attention; rebuild it with `python -m micromix_amd.build --force`")
    return lib


def kv_move_rows(kv_data, kv_param, kv_indptr, kv_indices, move_indptr, src_pos, dst_pos):
    """Within each sequence of a paged cache, move token rows from one logical position to another, for every layer, K and V, every
    head, in place; returns None.  Bytes only (codes and, for int4 / fp8, the fp16 params): no dequantization.

    Sequence b's moves are m in [move_indptr[b], move_indptr[b + 1]): the row at position src_pos[m] goes to position dst_pos[m], a
    position being row pos % P of page kv_indices[kv_indptr[b] + pos // P].  All sources of a sequence are read before any of its
    destinations is written, so a destination may be another move's source -- what packing the accepted path of a tree draft down to
    contiguous positions needs (PagedKVCache.accept).  At most 64 moves per sequence are performed; a move with src == dst, a position
    outside the pages the sequence lists or a page index outside the cache is skipped.  The destinations of a sequence must be pairwise
    distinct, and no page written may be listed by another sequence with moves in the call (include/micromix_hip.h, mm_kv_move_rows).
    move_indptr [B + 1], src_pos, dst_pos: int32 device tensors.  Runs on the current stream, capture-safe."""
    lib = _tree_lib()
    if kv_param is not None:
        kv_data = _kv_bytes(kv_data)
    if not (isinstance(kv_data, torch.Tensor) and kv_data.is_cuda):
        _check_tensor(kv_data, "kv_data", torch.uint8 if kv_param is not None else torch.bfloat16)
    dev = kv_data.device
    kind, max_pages, L, Hkv, P, kv_data = _kv_geometry(kv_data, kv_param, dev.index)
    for n, t in (("kv_indptr", kv_indptr), ("kv_indices", kv_indices), ("move_indptr", move_indptr), ("src_pos", src_pos), ("dst_pos", dst_pos)):
        if not _ok(t, torch.int32, dev.index):
            _check_tensor(t, n, torch.int32, dev)
        if t.dim() != 1:
            raise RuntimeError(f"{n} must be one-dimensional")
    B = kv_indptr.numel() - 1
    if B < 0 or move_indptr.numel() != B + 1:
        raise RuntimeError("kv_indptr and move_indptr must both have B + 1 entries")
    if src_pos.numel() != dst_pos.numel():
        raise RuntimeError("src_pos and dst_pos must be of one length")
    with _on_device(dev.index):
        st = lib.mm_kv_move_rows(_ptr(kv_data), _ptr(kv_param) if kv_param is not None else None, kind, max_pages, L, Hkv, P, 128,
                                 _ptr(kv_indptr), _ptr(kv_indices), B, _ptr(move_indptr), _ptr(src_pos), _ptr(dst_pos), src_pos.numel(),
                                 _stream_ptr(dev))
    if st:
        _lib.check(st, "kv_move_rows")


def _verify_lib():
    lib = _lib.load()
    if not hasattr(lib, "mm_verify_greedy"):
        raise _lib.MicroMixLibraryError("libmicromix_hip.so has no mm_argmax_rows / mm_verify_greedy: it was built before draft "
                                        "verification; rebuild it with `python -m micromix_amd.build --force`")
    return lib


def argmax_rows_workspace_bytes(rows, vocab):
    """bytes of workspace `argmax_rows` needs for bf16 logits [rows, vocab]; 0 when a row is one part (vocab <= MM_ARGMAX_CHUNK)"""
    return int(_verify_lib().mm_argmax_rows_workspace_bytes(int(rows), int(vocab)))


def argmax_rows(logits, *, out=None, workspace=None):
    """The index of each row's maximum: logits bf16 [rows, vocab] on the device, last stride 1, any row stride >= vocab (a slice
    logits[:, :V] of a padded lm_head output, at any 2-byte-aligned offset, is taken as it is: nothing is copied).  Returns int32 [rows]
    (`out` when given).  The order is torch.argmax's on the CPU: any NaN is greater than +inf, +0 == -0, the lowest index among equal
    maxima wins.  vocab <= 2^20, rows <= 65535.  workspace: a contiguous device tensor of `argmax_rows_workspace_bytes(rows, vocab)`
    bytes, uninitialised, allocated when needed and not given (under graph capture pass one).  Runs on the current stream,
    capture-safe."""
    lib = _verify_lib()
    if not isinstance(logits, torch.Tensor):
        raise TypeError("logits must be a torch.Tensor")
    if logits.dtype is not torch.bfloat16:
        raise TypeError(f"logits must be torch.bfloat16, got {logits.dtype}")
    if not logits.is_cuda:
        raise RuntimeError("logits must be a device tensor (HIP); the MicroMix ops have no CPU path")
    if logits.dim() != 2 or logits.size(1) < 1:
        raise RuntimeError("logits must be [rows, vocab] with vocab >= 1")
    rows, vocab = logits.shape
    if vocab > 1 and logits.stride(1) != 1:
        raise RuntimeError("logits must have unit stride along the vocabulary (the rows may be any distance >= vocab apart)")
    ld = logits.stride(0) if rows > 1 else vocab
    if ld < vocab:
        raise RuntimeError(f"logits rows overlap: row stride {ld} < vocab {vocab}")
    dev = logits.device
    if out is None:
        out = torch.empty((rows,), dtype=torch.int32, device=dev)
    elif not _ok(out, torch.int32, dev.index) or out.dim() != 1 or out.numel() != rows:
        _check_tensor(out, "out", torch.int32, dev)
        raise RuntimeError(f"out must be int32 [{rows}]")
    workspace, ws_args = _kv_workspace(workspace, argmax_rows_workspace_bytes(rows, vocab), dev)
    with _on_device(dev.index):
        st = lib.mm_argmax_rows(_ptr(logits), rows, vocab, ld, _ptr(out), *ws_args, _stream_ptr(dev))
    if st:
        _lib.check(st, "argmax_rows")
    return out


def _sample_lib():
    lib = _lib.load()
    if not hasattr(lib, "mm_sample_rows"):
        raise _lib.MicroMixLibraryError("libmicromix_hip.so has no mm_sample_rows: it was built before the sampler; rebuild it with "
                                        "`python -m micromix_amd.build --force`")
    return lib


def sample_rows_workspace_bytes(rows, vocab):
    """bytes of workspace `sample_rows` needs for bf16 logits [rows, vocab]: 3 KiB per part of MM_ARGMAX_CHUNK columns of every row
    and 2 KiB per row"""
    return int(_sample_lib().mm_sample_rows_workspace_bytes(int(rows), int(vocab)))


def _row_param(value, name, dtype, rows, dev):
    """a per-row parameter of `sample_rows`: None, a device tensor [rows] of `dtype`, or -- outside graph capture -- a Python number,
    broadcast to one"""
    if value is None:
        return None
    if isinstance(value, torch.Tensor):
        if not _ok(value, dtype, dev.index) or value.dim() != 1 or value.numel() != rows:
            _check_tensor(value, name, dtype, dev)
            raise RuntimeError(f"{name} must be {dtype} [{rows}], one entry per row")
        return value
    if isinstance(value, bool) or not isinstance(value, (int, float)):
        raise TypeError(f"{name} must be None, a number or a {dtype} device tensor [{rows}], got {type(value).__name__}")
    if dtype is torch.int32 and not isinstance(value, int):
        raise TypeError(f"{name} must be an int or a torch.int32 device tensor [{rows}], got {type(value).__name__}")
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"{name}: a Python number would be uploaded during graph capture; pass a {dtype} device tensor [{rows}]")
    if dtype is torch.int32:
        value = min(max(value, -(1 << 31)), (1 << 31) - 1)
    return torch.full((rows,), value, dtype=dtype, device=dev)


def sample_rows(logits, u, *, temperature=None, top_k=None, top_p=None, min_p=None, out=None, workspace=None):
    """One token per row, drawn under temperature, top-k, top-p and min-p: logits bf16 [rows, vocab] on the device as `argmax_rows`
    takes them (any row stride >= vocab, any 2-byte-aligned offset), u fp32 [rows] uniform in [0, 1) -- `torch.rand`, which captures;
    the library draws no random numbers.  Returns int32 [rows] (`out` when given), ready for `verify_greedy` / `verify_launch` as
    target_tok: the accepted path and the bonus token are then distributed as the target model's.

    temperature, top_p, min_p: fp32 [rows], top_k: int32 [rows], device tensors read by the kernels only, so one captured graph serves
    any mix of requests rewritten in place; None: temperature 1, that filter off; a Python number is broadcast to a tensor (outside
    capture only).  Per row: temperature <= 0 or NaN, or a row whose maximum is NaN or infinite, gives exactly `argmax_rows`' answer.
    Otherwise w_i = exp((l_i - max) / T); tokens of equal logit form a class and every filter keeps whole classes in descending
    order: top_k the shortest prefix with >= k tokens (1 <= k < vocab, else off), top_p the shortest prefix with mass >= p times
    top-k's (p < 1; p <= 0 keeps the top class), min_p the classes with w >= q (0 < q <= 1); the kept set is the shortest of the
    three; the answer is the first kept index whose cumulative kept mass exceeds u * Z (include/micromix_hip.h, mm_sample_rows).  The
    result is a function of the inputs alone: the same bits on every run.  vocab <= 2^20, rows <= 65535.  workspace: a contiguous
    device tensor of `sample_rows_workspace_bytes(rows, vocab)` bytes, uninitialised, allocated when not given (under graph capture
    pass one).  Runs on the current stream, capture-safe."""
    lib = _sample_lib()
    if not isinstance(logits, torch.Tensor):
        raise TypeError("logits must be a torch.Tensor")
    if logits.dtype is not torch.bfloat16:
        raise TypeError(f"logits must be torch.bfloat16, got {logits.dtype}")
    if not logits.is_cuda:
        raise RuntimeError("logits must be a device tensor (HIP); the MicroMix ops have no CPU path")
    if logits.dim() != 2 or logits.size(1) < 1:
        raise RuntimeError("logits must be [rows, vocab] with vocab >= 1")
    rows, vocab = logits.shape
    if vocab > 1 and logits.stride(1) != 1:
        raise RuntimeError("logits must have unit stride along the vocabulary (the rows may be any distance >= vocab apart)")
    ld = logits.stride(0) if rows > 1 else vocab
    if ld < vocab:
        raise RuntimeError(f"logits rows overlap: row stride {ld} < vocab {vocab}")
    dev = logits.device
    if u is None or not isinstance(u, torch.Tensor):
        raise TypeError(f"u must be a torch.float32 device tensor [{rows}] (torch.rand), got {type(u).__name__}")
    u = _row_param(u, "u", torch.float32, rows, dev)
    temperature = _row_param(temperature, "temperature", torch.float32, rows, dev)
    top_k = _row_param(top_k, "top_k", torch.int32, rows, dev)
    top_p = _row_param(top_p, "top_p", torch.float32, rows, dev)
    min_p = _row_param(min_p, "min_p", torch.float32, rows, dev)
    if out is None:
        out = torch.empty((rows,), dtype=torch.int32, device=dev)
    elif not _ok(out, torch.int32, dev.index) or out.dim() != 1 or out.numel() != rows:
        _check_tensor(out, "out", torch.int32, dev)
        raise RuntimeError(f"out must be int32 [{rows}]")
    workspace, ws_args = _kv_workspace(workspace, sample_rows_workspace_bytes(rows, vocab), dev)
    opt = lambda t: _ptr(t) if t is not None else None
    with _on_device(dev.index):
        st = lib.mm_sample_rows(_ptr(logits), rows, vocab, ld, _ptr(u), opt(temperature), opt(top_k), opt(top_p), opt(min_p), _ptr(out),
                                *ws_args, _stream_ptr(dev))
    if st:
        _lib.check(st, "sample_rows")
    return out


def verify_greedy(target_tok, draft_tok, root_tok, qo_indptr, kv_indptr, last_page_len, page_size, *, tree_mask=None, result=None,
                  move_src=None, move_dst=None):
    """Greedy (exact-match) verification of tree or chain drafts, one wave per sequence; returns (result, move_src, move_dst).

    Sequence b has the n = qo_indptr[b + 1] - qo_indptr[b] draft nodes of rows qo_indptr[b] .. : draft_tok[t] is a node's token,
    target_tok[t] the token the target model picks after it (`argmax_rows` or `sample_rows` of its logits), root_tok[b] the token
    picked after the last committed one.  tree_mask: the int64 words of `paged_prefill(tree_mask=)` -- a node's parent is the highest set
    bit below its own -- or None for chains.  Starting from root_tok[b], the walk takes the lowest-numbered child of the node just taken
    whose token is the one wanted, until there is none.  result int32 [B, 66]: [0] the path's length k, [1] the bonus token (the
    target's choice after the last node taken; root_tok[b] when nothing matched), [2 : 2 + k] the path, the rest -1.  A sequence with
    n > 64 or root_tok[b] < 0 is a prompt chunk and keeps all: [0] = n, [1] = target_tok of its last row (-1 for n = 0), path entries -1.
    move_src, move_dst int32 [T], laid over qo_indptr: pass them on as `kv_move_rows(..., move_indptr=qo_indptr, move_src, move_dst)`
    to pack each path down to the positions base_b .. base_b + k - 1 (base_b = len_b - n, len_b from kv_indptr / last_page_len /
    page_size).  Every element of the three outputs is written.  All tensors are int32 on one device (token ids as int64 are refused:
    convert them with .to(torch.int32)).  Runs on the current stream, capture-safe (include/micromix_hip.h, mm_verify_greedy)."""
    lib = _verify_lib()
    ints = (("target_tok", target_tok), ("draft_tok", draft_tok), ("root_tok", root_tok), ("qo_indptr", qo_indptr), ("kv_indptr", kv_indptr),
            ("last_page_len", last_page_len))
    for n, t in ints:                                      # what torch.argmax and a tokenizer hand over: say what to do about it
        if isinstance(t, torch.Tensor) and t.dtype is torch.int64:
            raise TypeError(f"{n} must be torch.int32, got torch.int64: convert it with {n}.to(torch.int32)")
    if not (isinstance(target_tok, torch.Tensor) and target_tok.is_cuda):
        _check_tensor(target_tok, "target_tok", torch.int32)
    dev = target_tok.device
    for n, t in ints:
        if not _ok(t, torch.int32, dev.index):
            _check_tensor(t, n, torch.int32, dev)
        if t.dim() != 1:
            raise RuntimeError(f"{n} must be one-dimensional")
    T, B = target_tok.numel(), root_tok.numel()
    if draft_tok.numel() != T:
        raise RuntimeError("target_tok and draft_tok must be of one length")
    if qo_indptr.numel() != B + 1 or kv_indptr.numel() != B + 1 or last_page_len.numel() != B:
        raise RuntimeError("qo_indptr and kv_indptr must have B + 1 entries and last_page_len B (B = root_tok.numel())")
    page_size = int(page_size)
    if page_size < 1:
        raise ValueError("page_size must be positive")
    if tree_mask is not None:
        if not _ok(tree_mask, torch.int64, dev.index):
            _check_tensor(tree_mask, "tree_mask", torch.int64, dev)
        if tree_mask.dim() != 1 or tree_mask.numel() != T:
            raise RuntimeError(f"tree_mask must be int64 [{T}], one word per row")
    if result is None:
        result = torch.empty((B, _lib.MM_VERIFY_STRIDE), dtype=torch.int32, device=dev)
    elif not _ok(result, torch.int32, dev.index) or tuple(result.shape) != (B, _lib.MM_VERIFY_STRIDE):
        _check_tensor(result, "result", torch.int32, dev)
        raise RuntimeError(f"result must be int32 [{B}, {_lib.MM_VERIFY_STRIDE}]")
    moves = []
    for n, t in (("move_src", move_src), ("move_dst", move_dst)):
        if t is None:
            t = torch.empty((T,), dtype=torch.int32, device=dev)
        elif not _ok(t, torch.int32, dev.index) or t.dim() != 1 or t.numel() != T:
            _check_tensor(t, n, torch.int32, dev)
            raise RuntimeError(f"{n} must be int32 [{T}]")
        moves.append(t)
    with _on_device(dev.index):
        st = lib.mm_verify_greedy(_ptr(target_tok), _ptr(draft_tok), _ptr(root_tok), _ptr(tree_mask) if tree_mask is not None else None,
                                  _ptr(qo_indptr), T, _ptr(kv_indptr), _ptr(last_page_len), page_size, B, _ptr(result), _ptr(moves[0]),
                                  _ptr(moves[1]), _stream_ptr(dev))
    if st:
        _lib.check(st, "verify_greedy")
    return result, moves[0], moves[1]


def _token_rows(t, name, heads):
    """(heads, token stride in elements) of q / k / v given as [T, H, 128] or [T, H * 128] whose rows lie contiguous within a token.
    Stride 0: any stride will do (at most one token); None: the tensor has to be copied (rows not contiguous, an odd stride, a
    misaligned pointer)"""
    if t.dim() == 3 and t.size(2) == 128:
        H, inner = t.size(1), t.stride(2) == 1 and (t.size(1) == 1 or t.stride(1) == 128)
    elif t.dim() == 2 and t.size(1) % 128 == 0 and t.size(1):
        H, inner = t.size(1) // 128, t.stride(1) == 1
    else:
        raise RuntimeError(f"{name} must be [T, H, 128] or [T, H * 128] bf16")
    if heads is not None and H != heads:
        raise RuntimeError(f"{name} has {H} heads, the cache has {heads}")
    stride = t.stride(0) if t.size(0) > 1 else 0
    ok = inner and (stride == 0 or stride >= H * 128) and stride % 2 == 0 and t.data_ptr() % 4 == 0
    return H, (stride if ok else None)


def rope_kv_append(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, q, k, v, cos, sin, append_indptr, layer_idx):
    """RoPE on q and k, then `kv_append` of (rotated k, v), in one launch; returns the rotated q, bf16 [T, Hq, 128] contiguous.

    q, k, v: bf16 [T, H, 128] or [T, H * 128].  Views of one packed [T, (Hq + 2 Hkv) * 128] projection (what FusedQLinear returns) are
    read in place; so are any three tensors with one common token stride.  Otherwise they are packed into one buffer first (one copy).
    cos, sin: bf16 [T, 128], or HF's [1, T, 128] / [bsz, q_len, 128] (flattened): row i belongs to flat token i; a row stride is honoured.
    RoPE is HF's apply_rotary_pos_emb in bf16 arithmetic, q * cos + rotate_half(q) * sin with every op rounded to bf16, bit for bit
    (include/micromix_hip.h, mm_rope_kv_append).  The cache receives exactly what kv_append(rope(k), v) writes; q is rotated for every
    token.  Page table, append_indptr and the three cache kinds (int4, fp8 e4m3, bf16) as in `kv_append`.  Runs on the current stream,
    capture-safe.
    """
    lib = _lib.load()
    dev, B, Hkv, kv_args = _kv_args(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, layer_idx)
    if not _ok(append_indptr, torch.int32, dev.index):
        _check_tensor(append_indptr, "append_indptr", torch.int32, dev)
    if append_indptr.numel() != B + 1:
        raise RuntimeError("append_indptr must have B + 1 entries")
    for n, t in (("q", q), ("k", k), ("v", v), ("cos", cos), ("sin", sin)):
        if not (isinstance(t, torch.Tensor) and t.dtype is torch.bfloat16 and t.is_cuda and t.get_device() == dev.index):
            _check_tensor(t, n, torch.bfloat16, dev)      # contiguity is not asked of these five
    Hq, sq = _token_rows(q, "q", None)
    _, sk = _token_rows(k, "k", Hkv)
    _, sv = _token_rows(v, "v", Hkv)
    T = q.size(0)
    if k.size(0) != T or v.size(0) != T:
        raise RuntimeError("q, k and v must hold the same T tokens")
    if Hq % Hkv:
        raise RuntimeError(f"the {Hq} query heads are not a multiple of the cache's {Hkv} kv heads")
    strides = {sq, sk, sv} - {0}
    if None in strides or len(strides) > 1 or max(strides, default=Hq * 128) < Hq * 128:
        packed = torch.cat([q.reshape(T, Hq * 128), k.reshape(T, Hkv * 128), v.reshape(T, Hkv * 128)], dim=1)
        q, k, v = packed[:, : Hq * 128], packed[:, Hq * 128: (Hq + Hkv) * 128], packed[:, (Hq + Hkv) * 128:]
        strides = {(Hq + 2 * Hkv) * 128}
    sq = max(strides, default=Hq * 128)
    if cos.shape != sin.shape or cos.dim() not in (2, 3) or cos.size(-1) != 128 or cos.numel() != T * 128:
        raise RuntimeError(f"cos and sin must both be [T = {T}, 128] (or [bsz, q_len, 128] with bsz * q_len = T) bf16")
    cos, sin = cos.reshape(T, 128), sin.reshape(T, 128)
    sc = cos.stride(0) if T > 1 else 128
    if not (cos.stride(1) == 1 and sin.stride(1) == 1 and (T <= 1 or sin.stride(0) == sc) and sc >= 128 and sc % 2 == 0
            and cos.data_ptr() % 4 == 0 and sin.data_ptr() % 4 == 0):
        cos, sin, sc = cos.contiguous(), sin.contiguous(), 128
    q_rot = torch.empty((T, Hq, 128), dtype=torch.bfloat16, device=dev)
    with _on_device(dev.index):
        st = lib.mm_rope_kv_append(*kv_args, _ptr(q), _ptr(k), _ptr(v), sq, Hq, _ptr(cos), _ptr(sin), sc, _ptr(append_indptr), T,
                                   _ptr(q_rot), _stream_ptr(dev))
    if st:
        _lib.check(st, "rope_kv_append")
    return q_rot


def _window(window):
    """HF's sliding_window as the C ABI takes it: None or 0 is no window (the un-windowed entry points), W >= 1 a window of W tokens"""
    window = 0 if window is None else int(window)
    if window < 0:
        raise ValueError("window must be None, 0 (no window) or a positive token count")
    return window


def paged_decode_workspace_bytes(B, Hq, Hkv, max_seq_len, window=None):
    """bytes of fp32 scratch paged_decode needs for this bound and window (0: one launch, no workspace)"""
    window = _window(window)
    if not window:
        return int(_lib.load().mm_paged_decode_workspace_bytes(int(B), int(Hq), int(Hkv), int(max_seq_len)))
    return int(_lib.load().mm_paged_decode_window_workspace_bytes(int(B), int(Hq), int(Hkv), int(max_seq_len), window))


def paged_decode(q, kv_data, kv_param, kv_indptr, kv_indices, last_page_len, layer_idx, max_seq_len, sm_scale=None, workspace=None, *,
                 window=None):
    """Single-token GQA attention over layer `layer_idx` of a paged cache: q bf16 [B, Hq, 128] -> o bf16 [B, Hq, 128].

    Query head h reads kv head h // (Hq / Hkv) (HF repeat_kv), every cached token, softmax in fp32 with sm_scale (default 1/sqrt(128));
    a sequence of length 0 gives zeros.  `max_seq_len` bounds the sequence lengths; the split over the tokens depends on it (and B,
    Hq, Hkv) only, so a captured graph stays valid while the sequences grow up to it.  `workspace` (uint8 / any device tensor of at
    least paged_decode_workspace_bytes(...) bytes) is allocated here when None -- pass one when capturing a graph.
    `window` = W (HF's sliding_window; None or 0: none): the query attends the last W tokens of its sequence, its own included.  Only
    these tokens are read, the split is laid over W tokens, and page-table entries below the window may be -1.
    The cache is int4, fp8 (e4m3) or bf16, told apart as in `kv_append`; over an fp8 cache the result equals, bit for bit, that over a
    bf16 cache holding the dequantized values.
    """
    lib = _lib.load()
    window = _window(window)
    dev, B, Hkv, kv_args = _kv_args(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, layer_idx, q)
    if q.dim() != 3 or q.size(0) != B or q.size(2) != 128:
        raise RuntimeError(f"q must be [B = {B}, Hq, 128] bf16")
    Hq = q.size(1)
    if Hq % Hkv:
        raise RuntimeError(f"the {Hq} query heads are not a multiple of the cache's {Hkv} kv heads")
    max_seq_len = int(max_seq_len)
    if max_seq_len < 0:
        raise RuntimeError("max_seq_len must be >= 0")
    need = paged_decode_workspace_bytes(B, Hq, Hkv, max_seq_len, window) if B else 0
    workspace, ws_args = _kv_workspace(workspace, need, dev)
    o = torch.empty((B, Hq, 128), dtype=torch.bfloat16, device=dev)
    scale = _sm_scale(sm_scale)
    with _on_device(dev.index):
        if window:
            st = lib.mm_paged_decode_window(_ptr(q), *kv_args, Hq, max_seq_len, scale, *ws_args, _ptr(o), _stream_ptr(dev), window)
        else:
            st = lib.mm_paged_decode(_ptr(q), *kv_args, Hq, max_seq_len, scale, *ws_args, _ptr(o), _stream_ptr(dev))
    if st:
        _lib.check(st, "paged_decode")
    return o


def _shared_lib():
    lib = _lib.load()
    if not hasattr(lib, "mm_paged_decode_shared"):
        raise _lib.MicroMixLibraryError("libmicromix_hip.so has no mm_paged_decode_shared: it was built before shared-prefix decode; "
                                        "rebuild it with `python -m micromix_amd.build --force`")
    return lib


def paged_decode_shared_workspace_bytes(B, Hq, Hkv, max_shared_len, max_suffix_len):
    """bytes of fp32 scratch paged_decode_shared needs for these bounds: the partials of its prefix and tail chunks (never 0 for B > 0
    and sizes the call takes; 0 for sizes it refuses)"""
    return int(_shared_lib().mm_paged_decode_shared_workspace_bytes(int(B), int(Hq), int(Hkv), int(max_shared_len), int(max_suffix_len)))


def paged_decode_shared(q, kv_data, kv_param, kv_indptr, kv_indices, last_page_len, layer_idx, group_indptr, group_members, shared_len,
                        max_shared_len, max_suffix_len, sm_scale=None, workspace=None, *, out=None):
    """`paged_decode` for a batch in which groups of sequences hold their leading pages in common: q bf16 [B, Hq, 128] -> o bf16
    [B, Hq, 128], the same function (every sequence attends all of its tokens), within the same budget but not the same bits.

    The shared tokens of a group are walked once per slab of 16 // (Hq // Hkv) members instead of once per member; each sequence's own
    tail is walked as in `paged_decode`.  group_indptr [B + 1], group_members [B], shared_len [B]: int32 device tensors.  Group j is
    group_members[group_indptr[j] : group_indptr[j + 1]], trailing unused groups are empty (group_indptr[j] = B), group_members is a
    permutation of range(B), and shared_len[b] -- the same for every member of a group, at most each member's length, any value, not
    only multiples of the page size -- counts the leading tokens b has on the same pages as its group (include/micromix_hip.h,
    mm_paged_decode_shared, also for what happens when the tensors break the rules: wrong results for those sequences, no access outside
    the tensors).  `PagedKVCache.share_groups()` derives one grouping from a page table; a caller who knows better (a beam tree whose
    branches share different depths) passes its own.
    `max_shared_len` bounds the shared counts, `max_suffix_len` the tails; the launches depend on them (and B, Hq, Hkv) only, so a
    captured graph stays valid while lengths and groups change within them.  `workspace` (at least
    paged_decode_shared_workspace_bytes(...) bytes; always needed) is allocated here when None -- pass one when capturing a graph.
    `out`: a bf16 [B, Hq, 128] tensor to write instead of a new one.  No sliding window.
    """
    lib = _shared_lib()
    dev, B, Hkv, kv_args = _kv_args(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, layer_idx, q)
    if q.dim() != 3 or q.size(0) != B or q.size(2) != 128:
        raise RuntimeError(f"q must be [B = {B}, Hq, 128] bf16")
    Hq = q.size(1)
    if Hq % Hkv:
        raise RuntimeError(f"the {Hq} query heads are not a multiple of the cache's {Hkv} kv heads")
    for n, t, size in (("group_indptr", group_indptr, B + 1), ("group_members", group_members, B), ("shared_len", shared_len, B)):
        if not _ok(t, torch.int32, dev.index):
            _check_tensor(t, n, torch.int32, dev)
        if t.dim() != 1 or t.numel() != size:
            raise RuntimeError(f"{n} must be a one-dimensional int32 tensor of {size} entries (B = {B})")
    max_shared_len, max_suffix_len = int(max_shared_len), int(max_suffix_len)
    if min(max_shared_len, max_suffix_len) < 0 or max(max_shared_len, max_suffix_len) > 1 << 29:
        raise RuntimeError("max_shared_len and max_suffix_len must lie in [0, 2^29]")
    need = paged_decode_shared_workspace_bytes(B, Hq, Hkv, max_shared_len, max_suffix_len) if B and Hq // Hkv <= 16 else 0
    workspace, ws_args = _kv_workspace(workspace, need, dev)
    if out is None:
        out = torch.empty((B, Hq, 128), dtype=torch.bfloat16, device=dev)
    elif not _ok(out, torch.bfloat16, dev.index) or tuple(out.shape) != (B, Hq, 128):
        _check_tensor(out, "out", torch.bfloat16, dev)
        raise RuntimeError(f"out must be [{B}, {Hq}, 128] bf16")
    scale = _sm_scale(sm_scale)
    with _on_device(dev.index):
        st = lib.mm_paged_decode_shared(_ptr(q), *kv_args, Hq, _ptr(group_indptr), _ptr(group_members), _ptr(shared_len), max_shared_len,
                                        max_suffix_len, scale, *ws_args, _ptr(out), _stream_ptr(dev))
    if st:
        _lib.check(st, "paged_decode_shared")
    return out


def paged_prefill_workspace_bytes(T, B, Hq, Hkv, max_seq_len, window=None):
    """bytes of fp32 scratch paged_prefill needs for T query tokens over B sequences within max_seq_len, under `window` (0: one launch,
    no workspace)"""
    window = _window(window)
    if not window:
        return int(_lib.load().mm_paged_prefill_workspace_bytes(int(T), int(B), int(Hq), int(Hkv), int(max_seq_len)))
    return int(_lib.load().mm_paged_prefill_window_workspace_bytes(int(T), int(B), int(Hq), int(Hkv), int(max_seq_len), window))


def paged_prefill(q, kv_data, kv_param, kv_indptr, kv_indices, last_page_len, qo_indptr, layer_idx, max_seq_len, sm_scale=None,
                  workspace=None, *, window=None, tree_mask=None):
    """Causal GQA attention of T new query tokens over layer `layer_idx` of a paged cache: q bf16 [T, Hq, 128] -> o bf16 [T, Hq, 128].

    qo_indptr (int32 [B + 1], qo_indptr[B] = T) splits the queries among the sequences, as kv_append's append_indptr does; pass the
    same array.  The page table already counts the new tokens, and the mask is aligned bottom-right: sequence b's j-th new token sits
    at position len_b - n_b + j and attends positions 0 .. that one.  Softmax in fp32 with sm_scale (default 1/sqrt(128)).
    `max_seq_len` bounds the sequence lengths; the grid and the split over the tokens depend on it (and T, B, Hq, Hkv) only, so a
    captured graph stays valid over later steps with the same T.  `workspace` (any contiguous device tensor of at least
    paged_prefill_workspace_bytes(...) bytes) is allocated here when None -- pass one when capturing a graph.
    `window` = W (HF's sliding_window; None or 0: none): the token at position p attends positions max(0, p - W + 1) .. p; the kv tiles
    below a query tile's windows are not read, and page-table entries below every window may be -1.
    `tree_mask` (int64 [T] device tensor, one word per query token; None: the causal mask): verification of a tree draft.  With
    base_b = len_b - n_b, sequence b's j-th new token attends every position below base_b and new slot base_b + i exactly when i <= j
    and bit i of its word is set (bits above j are ignored; set bit j for a token to attend itself).  A sequence with more than 64 new
    tokens ignores its words and is attended causally.  Words (2 << j) - 1 give the bits of the causal call.  No window form: `window`
    together with `tree_mask` is a ValueError.  The tensor is read by the kernel only, so a captured graph replays with other trees
    written into it.  `PagedKVCache.tree_mask` builds the words from parent indices.
    The cache is int4, fp8 (e4m3) or bf16, told apart as in `kv_append`; fp8 runs p.V on bf16(p * scale_v) times the codes, as int4.
    """
    lib = _lib.load() if tree_mask is None else _tree_lib()
    window = _window(window)
    if window and tree_mask is not None:
        raise ValueError("paged_prefill has no sliding-window form of the tree mask: pass window or tree_mask, not both")
    dev, B, Hkv, kv_args = _kv_args(kv_data, kv_param, kv_indptr, kv_indices, last_page_len, layer_idx, q)
    if not _ok(qo_indptr, torch.int32, dev.index):
        _check_tensor(qo_indptr, "qo_indptr", torch.int32, dev)
    if qo_indptr.numel() != B + 1:
        raise RuntimeError("qo_indptr must have B + 1 entries (B = last_page_len.numel())")
    if q.dim() != 3 or q.size(2) != 128:
        raise RuntimeError("q must be [T, Hq, 128] bf16, T = qo_indptr[-1]")
    T, Hq = q.size(0), q.size(1)
    if Hq % Hkv:
        raise RuntimeError(f"the {Hq} query heads are not a multiple of the cache's {Hkv} kv heads")
    if tree_mask is not None:
        if not _ok(tree_mask, torch.int64, dev.index):
            _check_tensor(tree_mask, "tree_mask", torch.int64, dev)
        if tree_mask.dim() != 1 or tree_mask.numel() != T:
            raise RuntimeError(f"tree_mask must be a one-dimensional int64 tensor of T = {T} words")
    max_seq_len = int(max_seq_len)
    if max_seq_len < 0:
        raise RuntimeError("max_seq_len must be >= 0")
    need = paged_prefill_workspace_bytes(T, B, Hq, Hkv, max_seq_len, window) if B and T else 0
    workspace, ws_args = _kv_workspace(workspace, need, dev)
    o = torch.empty((T, Hq, 128), dtype=torch.bfloat16, device=dev)
    scale = _sm_scale(sm_scale)
    with _on_device(dev.index):
        if tree_mask is not None:
            st = lib.mm_paged_prefill_tree(_ptr(q), _ptr(qo_indptr), T, *kv_args, Hq, max_seq_len, scale, *ws_args, _ptr(o),
                                           _stream_ptr(dev), _ptr(tree_mask))
        elif window:
            st = lib.mm_paged_prefill_window(_ptr(q), _ptr(qo_indptr), T, *kv_args, Hq, max_seq_len, scale, *ws_args, _ptr(o),
                                             _stream_ptr(dev), window)
        else:
            st = lib.mm_paged_prefill(_ptr(q), _ptr(qo_indptr), T, *kv_args, Hq, max_seq_len, scale, *ws_args, _ptr(o), _stream_ptr(dev))
    if st:
        _lib.check(st, "paged_prefill")
    return o


# ---- sparse MoE block (include/micromix_hip.h, mm_moe_*; micromix_amd/moe.py assembles the block) ----

def _moe_tensor(t, name, dtype, dev, shape=None):
    if not _ok(t, dtype, dev.index):
        _check_tensor(t, name, dtype, dev)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{name} must be {list(shape)}, got {list(t.shape)}")
    return t


def moe_route(logits, top_k, *, topk_ids=None, topk_w=None):
    """Top-k routing of the gate logits: logits bf16 [T, E] -> (topk_ids int32 [T, top_k], topk_w bf16 [T, top_k]).

    Not an export of the reference module; the same numbers as its softmax(float) -> topk -> renormalise -> cast
    (qMixtralLayer.py:422-426): the top_k largest logits in descending order, equal logits in ascending expert index (torch.topk
    leaves ties unspecified), w_j = exp(l_j - max) / sum over the selected, in fp32, rounded to bf16.  1 <= top_k <= 8,
    top_k <= E <= 64.  Outputs are allocated unless passed in.  Runs on the current stream, capture-safe.
    """
    lib = _lib.load()
    if not (isinstance(logits, torch.Tensor) and logits.is_cuda and _ok(logits, torch.bfloat16, logits.get_device())):
        _check_tensor(logits, "logits", torch.bfloat16)
    if logits.dim() != 2:
        raise RuntimeError("logits must be [T, E] bf16")
    dev, (T, E), top_k = logits.device, logits.shape, int(top_k)
    topk_ids = torch.empty((T, top_k), dtype=torch.int32, device=dev) if topk_ids is None else _moe_tensor(topk_ids, "topk_ids", torch.int32, dev, (T, top_k))
    topk_w = torch.empty((T, top_k), dtype=torch.bfloat16, device=dev) if topk_w is None else _moe_tensor(topk_w, "topk_w", torch.bfloat16, dev, (T, top_k))
    with _on_device(dev.index):
        st = lib.mm_moe_route(_ptr(logits), T, E, top_k, _ptr(topk_ids), _ptr(topk_w), _stream_ptr(dev))
    if st:
        _lib.check(st, "moe_route")
    return topk_ids, topk_w


def moe_plan(topk_ids, num_experts, *, expert_offsets=None, sorted_token=None, slot_of=None):
    """The dispatch plan of routed tokens: topk_ids int32 [T, top_k] -> (expert_offsets int32 [E + 1], sorted_token int32 [T * top_k],
    slot_of int32 [T, top_k]), a stable counting sort of the (token, k-slot) pairs by expert.

    Expert e owns the slots [expert_offsets[e], expert_offsets[e + 1]); within an expert the slots run by ascending token;
    sorted_token[s] is the token of slot s, slot_of[t, j] the slot of token t's j-th choice.  An id outside [0, E) is not counted and
    gets slot_of = -1; the slots left over then hold sorted_token = -1.  Deterministic; runs on the current stream, capture-safe.
    """
    lib = _lib.load()
    if not (isinstance(topk_ids, torch.Tensor) and topk_ids.is_cuda and _ok(topk_ids, torch.int32, topk_ids.get_device())):
        _check_tensor(topk_ids, "topk_ids", torch.int32)
    if topk_ids.dim() != 2:
        raise RuntimeError("topk_ids must be [T, top_k] int32")
    dev, (T, top_k), E = topk_ids.device, topk_ids.shape, int(num_experts)
    i32 = torch.int32
    if expert_offsets is None:      # without tokens the entry does no device work: the offsets are all zero then
        expert_offsets = (torch.empty if T else torch.zeros)((max(E, 0) + 1,), dtype=i32, device=dev)
    else:
        _moe_tensor(expert_offsets, "expert_offsets", i32, dev, (E + 1,))
        if T == 0:
            expert_offsets.zero_()
    sorted_token = torch.empty((T * top_k,), dtype=i32, device=dev) if sorted_token is None else _moe_tensor(sorted_token, "sorted_token", i32, dev, (T * top_k,))
    slot_of = torch.empty((T, top_k), dtype=i32, device=dev) if slot_of is None else _moe_tensor(slot_of, "slot_of", i32, dev, (T, top_k))
    with _on_device(dev.index):
        st = lib.mm_moe_plan(_ptr(topk_ids), T, E, top_k, _ptr(expert_offsets), _ptr(sorted_token), _ptr(slot_of), _stream_ptr(dev))
    if st:
        _lib.check(st, "moe_plan")
    return expert_offsets, sorted_token, slot_of


def moe_gather(x, sorted_token, *, out=None):
    """x bf16 [T, H], sorted_token int32 [n_rows] -> x_sorted bf16 [n_rows, H] with x_sorted[s] = x[sorted_token[s]] (H a multiple
    of 8).  A row whose sorted_token lies outside [0, T) is left as it was (uninitialised in an output allocated here).  Runs on the
    current stream, capture-safe."""
    lib = _lib.load()
    if not (isinstance(x, torch.Tensor) and x.is_cuda and _ok(x, torch.bfloat16, x.get_device())):
        _check_tensor(x, "x", torch.bfloat16)
    if x.dim() != 2:
        raise RuntimeError("x must be [T, H] bf16")
    dev, (T, H) = x.device, x.shape
    _moe_tensor(sorted_token, "sorted_token", torch.int32, dev)
    n_rows = sorted_token.numel()
    out = torch.empty((n_rows, H), dtype=torch.bfloat16, device=dev) if out is None else _moe_tensor(out, "out", torch.bfloat16, dev, (n_rows, H))
    with _on_device(dev.index):
        st = lib.mm_moe_gather(_ptr(x), _ptr(sorted_token), T, n_rows, H, _ptr(out), _stream_ptr(dev))
    if st:
        _lib.check(st, "moe_gather")
    return out


def moe_combine(y_sorted, topk_ids, topk_w, slot_of, *, out=None):
    """The weighted sum of every token's expert outputs: y_sorted bf16 [T * top_k, H] (rows in plan order), topk_ids int32, topk_w bf16,
    slot_of int32, all [T, top_k] -> out bf16 [T, H].

    Per token its entries are taken in ascending expert id, c = bf16(y * w), acc = bf16(acc + c) from +0.0: bit for bit what the
    reference's zeros + index_add_ expert by expert leaves (qMixtralLayer.py:428-450), whatever order topk_ids lists the experts in.
    Entries with slot_of = -1 are skipped; every row of out is written.  Runs on the current stream, capture-safe.
    """
    lib = _lib.load()
    if not (isinstance(y_sorted, torch.Tensor) and y_sorted.is_cuda and _ok(y_sorted, torch.bfloat16, y_sorted.get_device())):
        _check_tensor(y_sorted, "y_sorted", torch.bfloat16)
    dev = y_sorted.device
    _moe_tensor(topk_ids, "topk_ids", torch.int32, dev)
    if topk_ids.dim() != 2 or y_sorted.dim() != 2 or y_sorted.size(0) != topk_ids.numel():
        raise RuntimeError("topk_ids must be [T, top_k] and y_sorted [T * top_k, H]")
    T, top_k = topk_ids.shape
    H = y_sorted.size(1)
    _moe_tensor(topk_w, "topk_w", torch.bfloat16, dev, (T, top_k))
    _moe_tensor(slot_of, "slot_of", torch.int32, dev, (T, top_k))
    out = torch.empty((T, H), dtype=torch.bfloat16, device=dev) if out is None else _moe_tensor(out, "out", torch.bfloat16, dev, (T, H))
    with _on_device(dev.index):
        st = lib.mm_moe_combine(_ptr(y_sorted), _ptr(topk_ids), _ptr(topk_w), _ptr(slot_of), T, top_k, H, _ptr(out), _stream_ptr(dev))
    if st:
        _lib.check(st, "moe_combine")
    return out


# ---- device-sized grouped launches: the expert quantizer and GEMM of a capturable MoE block (mm_moe_quantize / mm_moe_matmul) ----

class MoEExpertTable:
    """`mm_moe_expert[E]` in device memory (include/micromix_hip.h) with the tensors it points to kept alive.  `tensor` int64 [E, 8]:
    per expert the addresses of (reorder_index, BN, BS, BO, SFBN, SFBS, SFBO, bias or 0).  Built once, by moe_expert_table."""
    __slots__ = ("tensor", "E", "N", "K", "split", "wmode", "has_bias", "_keep")


def moe_expert_table(reorder_indices, Bs, KN, KS, KO, biases=None):
    """One table per layer of the experts: reorder_indices[e] int16 [K], Bs[e] = (BN, BS, BO, SFBN, SFBS, SFBO) as matmul_grouped takes
    them, biases[e] bf16 [N] or None.  All experts share N, the (KN, KS, KO) split and the weight mode.  The addresses are copied to the
    device here -- build the table once (SparseMoEBlock.__init__), never per call."""
    E = len(Bs)
    if not (1 <= E <= 64) or len(reorder_indices) != E or (biases is not None and len(biases) != E):
        raise ValueError("1 <= E <= 64 experts, one reorder index (and bias entry) each")
    KN, KS, KO = int(KN), int(KS), int(KO)
    K = KN + KS + KO
    _check_split(KN, KS, KO, None, "moe_expert_table")
    dev = Bs[0][0].device
    index, u8 = dev.index, torch.uint8
    N = Bs[0][0].size(0)
    same = Bs[0][1].size(1) == KS // 4 * 3 and Bs[0][2].size(1) == KO          # (as matmul_grouped tells the weight mode)
    wmode = _lib.MM_W_MATCH if same else _lib.MM_W_FP4
    wb = (KN // 2, KS // 4 * 3 if same else KS // 2, KO if same else KO // 2)
    if tuple(tuple(t.shape) for t in Bs[0][:3]) != tuple((N, w) for w in wb):
        raise RuntimeError("the packed weights of expert 0 do not match the split in either weight mode")
    shapes = tuple(tuple(t.shape) for t in Bs[0])
    rows, keep = [], []
    for e, (idx, B) in enumerate(zip(reorder_indices, Bs)):
        if not _ok(idx, torch.int16, index) or idx.numel() != K:
            _check_tensor(idx, f"reorder_index[{e}]", torch.int16, dev)
            raise RuntimeError(f"expert {e}: the reorder index must have {K} entries")
        for t in B:
            if not _ok(t, u8, index):
                _check_tensor(t, f"expert {e} weight operand", u8, dev)
        if tuple(tuple(t.shape) for t in B[:3]) != shapes[:3] or any(t.numel() < _sf_bytes_w(N, k) for t, k in zip(B[3:], (KN, KS, KO))):
            raise RuntimeError(f"expert {e}: packed weights do not match N / split / weight mode of expert 0")
        bias = biases[e] if biases is not None else None
        if bias is not None and (not _ok(bias, torch.bfloat16, index) or bias.numel() != N):
            raise RuntimeError(f"expert {e}: bias must be a bfloat16 tensor with N elements")
        rows.append([idx.data_ptr()] + [t.data_ptr() if t.numel() else 0 for t in B] + [bias.data_ptr() if bias is not None else 0])
        keep.append((idx, B, bias))
    tab = MoEExpertTable()
    tab.tensor = torch.tensor(rows, dtype=torch.int64).to(dev)
    tab.E, tab.N, tab.K, tab.split, tab.wmode, tab._keep = E, N, K, (KN, KS, KO), wmode, keep
    tab.has_bias = biases is not None and any(b is not None for b in biases)
    return tab


def moe_sf_bytes(n, E, Kseg):
    """bytes of a packed scale tensor for n rows of E experts: n // 128 + E tiles of 128 rows (include/micromix_hip.h)"""
    return (n // 128 + E) * 128 * (Kseg // 32)


def _moe_outputs(out, n, E, widths, split, dev):
    """the 6-tuple a MoE quantizer fills: allocated, or the caller's `out` checked"""
    u8 = torch.uint8
    if out is None:
        return tuple(torch.empty((n, w), dtype=u8, device=dev) for w in widths) + \
            tuple(torch.empty((moe_sf_bytes(n, E, k),), dtype=u8, device=dev) for k in split)
    for t, w in zip(out[:3], widths):
        _moe_tensor(t, "packed output", u8, dev, (n, w))
    for t, k in zip(out[3:], split):
        if _moe_tensor(t, "scale output", u8, dev).numel() < moe_sf_bytes(n, E, k):
            raise RuntimeError("a scale output is smaller than moe_sf_bytes(n, E, Kseg)")
    return out


def moe_quantize(src, row_of_slot, expert_offsets, table, n=None, *, mode="x", out=None):
    """The expert quantizer with the row counts read on the device: for every slot s that an expert owns (expert_offsets int32 [E + 1],
    moe_plan's), row row_of_slot[s] of src bf16 [rows, K] -- row s itself with row_of_slot=None -- quantized with that expert's reorder
    index (table: moe_expert_table).  Returns ONE 6-tuple (oN, oS, oO, sfN, sfS, sfO) for all experts: packed rows in slot order
    [n, .], scale tensors of moe_sf_bytes(n, E, Kseg) bytes with expert e's run at tile expert_offsets[e] // 128 + e; bytes of slots and
    tiles that no expert owns are left as they were.  n defaults to len(row_of_slot) (or src's rows).  mode "x" (mixed) or "w4".
    Byte for byte reorder_quantize_x_grouped's per-expert tensors laid end to end.  No host sync; capture-safe."""
    lib = _lib.load()
    if not (isinstance(src, torch.Tensor) and src.is_cuda and _ok(src, torch.bfloat16, src.get_device())):
        _check_tensor(src, "src", torch.bfloat16)
    if src.dim() != 2:
        raise RuntimeError("src must be [rows, K] bf16")
    dev, (src_rows, K) = src.device, src.shape
    if mode not in ("x", "w4"):
        raise ValueError("mode must be 'x' or 'w4'")
    w4 = mode == "w4"
    E, (KN, KS, KO) = table.E, table.split
    if K != table.K:
        raise RuntimeError(f"src must be [rows, {table.K}]")
    _moe_tensor(expert_offsets, "expert_offsets", torch.int32, dev, (E + 1,))
    if row_of_slot is not None:
        _moe_tensor(row_of_slot, "row_of_slot", torch.int32, dev)
        n = row_of_slot.numel() if n is None else int(n)
        if row_of_slot.numel() < n:
            raise RuntimeError("row_of_slot must have n entries")
    else:
        n = src_rows if n is None else int(n)
    out = _moe_outputs(out, n, E, (KN // 2, KS // 2 if w4 else KS // 4 * 3, KO // 2 if w4 else KO), (KN, KS, KO), dev)
    with _on_device(dev.index):
        st = lib.mm_moe_quantize(_ptr(src), _ptr(row_of_slot) if row_of_slot is not None else None, _ptr(expert_offsets), _ptr(table.tensor), E, n,
                                 src_rows, K, KN, KS, KO, _lib.MM_QUANT_W4 if w4 else _lib.MM_QUANT_MIXED, *(_ptr(t) for t in out), _stream_ptr(dev))
    if st:
        _lib.check(st, "moe_quantize")
    return tuple(out)


def moe_activate_quantize(a, b, expert_offsets, table, *, out=None, h_out=None):
    """The experts' activation and the quantizer of their down-projection in one launch: a, b bf16 [n, K] in slot order (the outputs of
    moe_matmul for w1 and w3), and for every slot s that an expert owns h[s] = bf16(bf16(silu(a[s])) * b[s]) -- torch's bf16
    `F.silu(a) * b` except where the device exp2 / rcp move a value across a bf16 rounding boundary (include/micromix_hip.h) --
    quantized as moe_quantize(h, None, expert_offsets, table) would.  Returns that 6-tuple, byte for byte; `out=` takes a 6-tuple to
    fill.  h_out: None, or a bf16 [n, K] tensor (not a or b) that also receives h.  Slots no expert owns are left as they were in
    every output.  Mixed mode only.  No host sync, no allocation sized by device data; capture-safe."""
    lib = _lib.load()
    if not (isinstance(a, torch.Tensor) and a.is_cuda and _ok(a, torch.bfloat16, a.get_device())):
        _check_tensor(a, "a", torch.bfloat16)
    if a.dim() != 2:
        raise RuntimeError("a must be [n, K] bf16")
    dev, (n, K) = a.device, a.shape
    _moe_tensor(b, "b", torch.bfloat16, dev, (n, K))
    E, (KN, KS, KO) = table.E, table.split
    if K != table.K:
        raise RuntimeError(f"a and b must be [n, {table.K}]")
    _moe_tensor(expert_offsets, "expert_offsets", torch.int32, dev, (E + 1,))
    if h_out is not None:
        _moe_tensor(h_out, "h_out", torch.bfloat16, dev, (n, K))
        if h_out.data_ptr() in (a.data_ptr(), b.data_ptr()) and n:
            raise RuntimeError("h_out must not be a or b")
    out = _moe_outputs(out, n, E, (KN // 2, KS // 4 * 3, KO), (KN, KS, KO), dev)
    with _on_device(dev.index):
        st = lib.mm_moe_activate_quantize(_ptr(a), _ptr(b), _ptr(expert_offsets), _ptr(table.tensor), E, n, K, KN, KS, KO, *(_ptr(t) for t in out),
                                          _ptr(h_out) if h_out is not None else None, _stream_ptr(dev))
    if st:
        _lib.check(st, "moe_activate_quantize")
    return tuple(out)


def moe_matmul_supported(max_rows, table):
    """False where moe_matmul would answer "unsupported configuration" (very long K: take matmul_grouped there)"""
    return bool(_lib.load().mm_moe_matmul_supported(int(max_rows), table.N, *table.split, table.wmode))


def moe_matmul(A, expert_offsets, table, max_rows, *, rounding="reference", out=None):
    """The expert GEMM with the row counts read on the device: A = moe_quantize's 6-tuple (mode "x"), out bf16 [n, N] with the rows of
    expert e = matmul_grouped's output for that expert (bit for bit wherever both split K over the same number of waves, and always when
    K <= 512: include/micromix_hip.h), weights and biases from `table`.  max_rows: a bound on any expert's
    rows that the caller vouches for (T in a MoE block); an expert with more rows is skipped, its rows of `out` left as they were, as
    are the rows from expert_offsets[E] on.  At most two launches, whatever E.  No host sync; capture-safe."""
    lib = _lib.load()
    if rounding not in ("reference", "fused"):
        _round_flags(rounding)
    flags = _lib.MM_ROUND_PER_SEGMENT if rounding == "reference" else _lib.MM_ROUND_ONCE
    dev = A[0].device
    E, N, (KN, KS, KO) = table.E, table.N, table.split
    n = A[0].size(0)
    u8 = torch.uint8
    for t, w in zip(A[:3], (KN // 2, KS // 4 * 3, KO)):
        _moe_tensor(t, "activation segment", u8, dev, (n, w))
    for t, k in zip(A[3:], (KN, KS, KO)):
        if _moe_tensor(t, "activation scales", u8, dev).numel() < moe_sf_bytes(n, E, k):
            raise RuntimeError("an activation scale tensor is smaller than moe_sf_bytes(n, E, Kseg)")
    _moe_tensor(expert_offsets, "expert_offsets", torch.int32, dev, (E + 1,))
    out = torch.empty((n, N), dtype=torch.bfloat16, device=dev) if out is None else _moe_tensor(out, "out", torch.bfloat16, dev, (n, N))
    with _on_device(dev.index):
        st = lib.mm_moe_matmul(*(_ptr(t) for t in A), _ptr(expert_offsets), _ptr(table.tensor), E, n, int(max_rows), N, KN, KS, KO, table.wmode,
                               flags, _ptr(out), _stream_ptr(dev))
    if st:
        _lib.check(st, "moe_matmul")
    return out


# ---- w1 | w3, silu * mul and w2's quantizer in one expert launch (mm_moe_gate_up_activate) ----

def permute_packed_rows(packed6, perm):
    """Rows of a packed weight (BN, BS, BO, SFBN, SFBS, SFBO) in another order: row j of the result is row perm[j] of the input.

    Weights are quantized per output row, so this is a pure byte shuffle, equal byte for byte to quantizing the row-permuted weight:
    the packed codes move as rows; a scale tensor is tiled per 128 rows, and inside a tile's 512-byte atom of one 128-column slab row
    r sits at (r & 31) * 16 + ((r >> 5) & 3) * 4 (sf_offset, csrc/mx_common.h).  The row count must be a multiple of 128 (whole scale
    tiles) and perm a permutation of it.  Plain torch on any device, CPU tensors included; returns new tensors."""
    n = packed6[0].size(0)
    perm = torch.as_tensor(perm).to(device=packed6[0].device, dtype=torch.long).reshape(-1)
    if n % 128 or perm.numel() != n or (n and not torch.equal(torch.sort(perm).values, torch.arange(n, device=perm.device))):
        raise ValueError("permute_packed_rows: the rows must be a multiple of 128 and perm a permutation of them")
    out = [t.index_select(0, perm) if t.numel() else t.clone() for t in packed6[:3]]
    for t in packed6[3:]:
        if t.numel() == 0:
            out.append(t.clone())
            continue
        if t.numel() % (n * 4):
            raise ValueError("permute_packed_rows: a scale tensor is not whole 128-row tiles of these rows")
        atoms = t.numel() // (n * 4)                                  # 128-column slabs of the segment
        rows = t.reshape(n // 128, atoms, 32, 4, 4).permute(0, 3, 2, 1, 4).reshape(n, atoms * 4)        # [row, its scale bytes]
        rows = rows.index_select(0, perm)
        out.append(rows.reshape(n // 128, 4, 32, atoms, 4).permute(0, 3, 2, 1, 4).reshape(-1).contiguous())
    return tuple(out)


def moe_gate_up_table(reorder_indices1, w1s, w3s, reorder_indices2, split1, split2, *, biases1=None, biases3=None):
    """The device table of `moe_gate_up_activate`: per expert ONE packed fp4 weight of N = 2 I rows made from w1s[e] and w3s[e] (the
    6-tuples moe_expert_table takes).  Row j of the gate half is w1 row reorder_indices2[e][j], row j of the up half is w3 row
    reorder_indices2[e][j] -- the expert's w2 reorder index moves into the weight, because the fused epilogue quantizes 128 consecutive
    features into one segment of w2's K split -- and the halves are interleaved per 128 rows (interleave_gate_up).  reorder_indices1[e]
    is the index of the first quantizer (w1's), split1 / split2 the (KN, KS, KO) splits of w1 and of w2.  Returns a MoEExpertTable with
    N = 2 I and no bias whose weights are NEW tensors that it keeps alive: while the originals stay in use elsewhere, the memory held
    for w1 / w3 doubles.  Raises ValueError for biases on w1 / w3, weights that are not fp4 (MM_W_FP4), I not a multiple of 128 or an
    entry of split2 that is not a multiple of 128 (or split2 not adding up to I)."""
    E = len(w1s)
    if not (1 <= E <= 64) or len(w3s) != E or len(reorder_indices1) != E or len(reorder_indices2) != E:
        raise ValueError("moe_gate_up_table: 1 <= E <= 64 experts with w1, w3 and both reorder indices each")
    if any(b is not None for bs in (biases1, biases3) if bs is not None for b in bs):
        raise ValueError("moe_gate_up_table: w1 / w3 must have no bias (the fused epilogue adds none)")
    KN, KS, KO = (int(k) for k in split1)
    split2 = tuple(int(k) for k in split2)
    I = w1s[0][0].size(0)
    if I < 128 or I % 128:
        raise ValueError(f"moe_gate_up_table: I = {I} must be a multiple of 128")
    if len(split2) != 3 or any(k < 0 or k % 128 for k in split2) or sum(split2) != I:
        raise ValueError(f"moe_gate_up_table: split2 = {split2} must be three non-negative multiples of 128 that add up to I = {I}")
    fp4 = ((I, KN // 2), (I, KS // 2), (I, KO // 2))
    Bs = []
    for e in range(E):
        for name, B in (("w1", w1s[e]), ("w3", w3s[e])):
            if tuple(tuple(t.shape) for t in B[:3]) != fp4:
                raise ValueError(f"moe_gate_up_table: expert {e}: {name} must be fp4 weights (MM_W_FP4) of [{I}, .] rows matching split1")
            if any(t.numel() < _sf_bytes_w(I, k) for t, k in zip(B[3:], (KN, KS, KO))):
                raise ValueError(f"moe_gate_up_table: expert {e}: a scale tensor of {name} holds fewer than _sf_bytes_w(I, Kseg) bytes")
        idx2 = reorder_indices2[e]
        if idx2.numel() != I:
            raise ValueError(f"moe_gate_up_table: expert {e}: w2's reorder index must have I = {I} entries")
        whole = lambda B: tuple(B[:3]) + tuple(t.reshape(-1)[:_sf_bytes_w(I, k)] for t, k in zip(B[3:], (KN, KS, KO)))
        Bs.append(interleave_gate_up(permute_packed_rows(whole(w1s[e]), idx2), permute_packed_rows(whole(w3s[e]), idx2)))
    tab = moe_expert_table(reorder_indices1, Bs, KN, KS, KO)
    tab.wmode = _lib.MM_W_FP4              # (moe_expert_table cannot tell the modes apart when KS = KO = 0)
    return tab


def _gate_up_split2(table, split2):
    DN, DS, DO = (int(k) for k in split2)
    if table.N % 256:
        raise RuntimeError("table must be a moe_gate_up_table (N = 2 I, I a multiple of 128)")
    _check_split(DN, DS, DO, table.N // 2, "moe_gate_up_activate")
    return DN, DS, DO


def moe_gate_up_activate_supported(max_rows, table, split2):
    """False where moe_gate_up_activate would refuse: max_rows < 1, a bad split, or a table whose weights are not fp4"""
    I = table.N // 2
    return table.N % 256 == 0 and bool(_lib.load().mm_moe_gate_up_activate_supported(int(max_rows), I, *table.split, *(int(k) for k in split2), table.wmode))


def moe_gate_up_activate_describe(table, n, split2=None):
    """which kernel family and how many workgroups moe_gate_up_activate launches for n rows on the current device"""
    return _lib.load().mm_moe_gate_up_activate_describe(table.E, int(n), table.N // 2).decode()


def moe_gate_up_activate(A, expert_offsets, table, max_rows, split2, *, rounding="reference", out=None):
    """Both up-projections of the experts, silu * mul and the quantizer of their down-projection in ONE launch: A = moe_quantize's
    6-tuple (mode "x", w1's split), table = moe_gate_up_table(..), split2 = w2's (KN, KS, KO).  Returns the 6-tuple that moe_matmul
    takes for w2 -- for every slot an expert of 1 .. max_rows rows owns byte for byte what
    `moe_activate_quantize(moe_matmul(A, .., w1), moe_matmul(A, .., w3), offsets, w2's table)` gives wherever moe_matmul runs the
    expert on the tiled kernels (more than 64 rows; below that it may add its fp32 partial sums in another order, include/micromix_hip.h).
    Scale bytes of rows past an expert's last inside its own 128-row tiles are unspecified; everything else outside the experts' rows
    and runs, and the rows of an expert above max_rows, are left as they were.  `out=` takes a 6-tuple to fill.  No host sync, no
    allocation sized by device data; capture-safe."""
    lib = _lib.load()
    if rounding not in ("reference", "fused"):
        _round_flags(rounding)
    flags = _lib.MM_ROUND_PER_SEGMENT if rounding == "reference" else _lib.MM_ROUND_ONCE
    dev = A[0].device
    E, (KN, KS, KO) = table.E, table.split
    DN, DS, DO = _gate_up_split2(table, split2)
    n = A[0].size(0)
    u8 = torch.uint8
    for t, w in zip(A[:3], (KN // 2, KS // 4 * 3, KO)):
        _moe_tensor(t, "activation segment", u8, dev, (n, w))
    for t, k in zip(A[3:], (KN, KS, KO)):
        if _moe_tensor(t, "activation scales", u8, dev).numel() < moe_sf_bytes(n, E, k):
            raise RuntimeError("an activation scale tensor is smaller than moe_sf_bytes(n, E, Kseg)")
    _moe_tensor(expert_offsets, "expert_offsets", torch.int32, dev, (E + 1,))
    out = _moe_outputs(out, n, E, (DN // 2, DS // 4 * 3, DO), (DN, DS, DO), dev)
    with _on_device(dev.index):
        st = lib.mm_moe_gate_up_activate(*(_ptr(t) for t in A), _ptr(expert_offsets), _ptr(table.tensor), E, n, int(max_rows), table.N // 2, KN, KS, KO,
                                         DN, DS, DO, flags, *(_ptr(t) for t in out), _stream_ptr(dev))
    if st:
        _lib.check(st, "moe_gate_up_activate")
    return tuple(out)
