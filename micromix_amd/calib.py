"""Calibration side inputs of the hot path: the on-disk format the reference's
`reorder_indices.py` writes and `model/main.py` reads, and the rule that produces it.

Files (reorder_indices.py:149-151, main.py:114-124), all `torch.save`d dicts keyed by
`layers.{i}.self_attn.{q,k,v,o}_proj.input` / `layers.{i}.mlp.{gate,up,down}_proj.input`
(Mixtral: `layers.{i}.block_sparse_moe.experts.{j}.{w1,w2,w3}.input`):
    saved/{model}_reorder_index_wikitext2.pt   key -> LongTensor[K]  (ascending argsort of the channel score)
    saved/{model}_p6_num_wikitext2.pt          key -> int (multiple of 128)
    saved/{model}_p8_num_wikitext2.pt          key -> int (multiple of 128)

`split_from_activations` restates reorder_indices.py:41-49,64-69,98-111 so that the same side inputs can be produced
from any activation sample (the reference needs HF weights + wikitext2, neither available offline).  It is a one-shot over
activations held in memory, with one mean over all of them and ratios in Python doubles.

`accumulate` and `Calibrator` are the reference's rule itself as a streaming reduction on the device (include/micromix_calib.h,
csrc/calib_stats.hip): per hooked forward pass one pass over the activation where it lies, the state per key K floats and two
integers, the channel score the maximum over passes of the per-pass mean (:44-47), the ratios in the reference's fp32 tensor
arithmetic (:106-110).  `Calibrator.finish` returns the dicts `save_calibration` takes."""
from __future__ import annotations

import math
import os
from typing import Dict, Tuple

import torch

from . import _lib
from ._args import _launch, _lib_with, _ptr, _stream_ptr, _tensor

SUFFIXES = ("reorder_index", "p6_num", "p8_num")


def file_names(model_name: str, dataset: str = "wikitext2") -> Tuple[str, str, str]:
    return tuple(f"{model_name}_{s}_{dataset}.pt" for s in SUFFIXES)


def load_calibration(directory: str, model_name: str, dataset: str = "wikitext2"):
    """-> (reorder_index, p6_nums, p8_nums) exactly as main.py:121-123 loads them."""
    paths = [os.path.join(directory, f) for f in file_names(model_name, dataset)]
    if not os.path.isfile(paths[0]):
        raise FileNotFoundError("reorder index file not found.")          # main.py:118
    reorder_index = torch.load(paths[0], weights_only=False)
    p6 = torch.load(paths[1], weights_only=False)
    p8 = torch.load(paths[2], weights_only=False)
    validate(reorder_index, p6, p8)
    return reorder_index, p6, p8


def save_calibration(directory: str, model_name: str, reorder_index: Dict[str, torch.Tensor], p6: Dict[str, int],
                     p8: Dict[str, int], dataset: str = "wikitext2"):
    validate(reorder_index, p6, p8)
    os.makedirs(directory, exist_ok=True)
    for f, obj in zip(file_names(model_name, dataset), (reorder_index, p6, p8)):
        torch.save(obj, os.path.join(directory, f))


def validate(reorder_index, p6, p8):
    for key, idx in reorder_index.items():
        k = idx.numel()
        if key not in p6 or key not in p8:
            raise KeyError(f"{key}: p6_num / p8_num entry missing")
        a, b = int(p6[key]), int(p8[key])
        if a % 128 or b % 128 or a < 0 or b < 0 or a + b > k or (k - a - b) % 128:
            raise ValueError(f"{key}: p6_num={a}, p8_num={b} must be multiples of 128 with p4 = K - p6 - p8 >= 0 (K={k})")
        if k > 32768:
            raise ValueError(f"{key}: K={k} does not fit the int16 reorder index of the kernels")
        if not torch.equal(torch.sort(idx.long()).values, torch.arange(k)):
            raise ValueError(f"{key}: reorder_index is not a permutation of range({k})")


def split_from_activations(x: torch.Tensor, lamda: float = 1.0):
    """x: [tokens, K] activations feeding one linear layer.  Returns (reorder_index LongTensor[K], p4, p6, p8).

    reorder_indices.py: channel score = mean |x| over tokens (:44, max over batches :47), ascending argsort (:66);
    per-token thresholds p4_thr = rowmax * 448/6/2^10 * lamda, p6_thr = rowmax * 448/28/2^6 * lamda (:103-104);
    ratios of elements below them (:106-108); p6/p8 rounded UP to multiples of 128 (:109-110)."""
    v = x.reshape(-1, x.shape[-1]).float().abs()
    k = v.shape[-1]
    order = torch.sort(v.mean(dim=0), descending=False).indices
    rowmax = v.max(dim=-1, keepdim=True)[0]
    p4_thr = rowmax * 448 / 6 / math.pow(2, 10) * lamda
    p6_thr = rowmax * 448 / 28 / math.pow(2, 6) * lamda
    p4_ratio = float((v < p4_thr).sum()) / v.numel()
    p6_ratio = float((v < p6_thr).sum()) / v.numel() - p4_ratio
    p8_ratio = 1 - p4_ratio - p6_ratio
    p6 = math.ceil(k * p6_ratio / 128) * 128
    p8 = math.ceil(k * p8_ratio / 128) * 128
    p6 = max(0, min(p6, k))
    p8 = max(0, min(p8, k - p6))
    return order, k - p6 - p8, p6, p8


def llama_keys(num_layers: int):
    """the dict keys QLlamaAttention / QLlamaMLP look up (qLlamaLayer.py:212-235, 336-355)."""
    for i in range(num_layers):
        for blk, projs in (("self_attn", ("q_proj", "k_proj", "v_proj", "o_proj")), ("mlp", ("gate_proj", "up_proj", "down_proj"))):
            for p in projs:
                yield f"layers.{i}.{blk}.{p}.input"


# ---- the streaming rule on the device ----

_CALIB = ("mm_calib_accumulate", "mm_calib_accumulate", "device calibration")
_DTYPES = {torch.bfloat16: 0, torch.float16: 1}


def _lamda(lamda) -> float:
    lamda = float(lamda)
    if not (0.0 < lamda < math.inf):
        raise ValueError("lamda must be finite and positive")
    return lamda


def _rows(x):
    """(x as [rows, K] with unit stride along K, elements between rows): a view wherever the kernel's alignment rules allow one (the
    first element and the row stride at multiples of 16 bytes), else a contiguous copy"""
    k = x.shape[-1]
    v = x if x.dim() == 2 else None
    if v is None and k:
        try:
            v = x.view(-1, k)
        except RuntimeError:        # no single row stride
            pass
    if v is not None:
        ld = v.stride(0) if v.shape[0] > 1 else k
        if v.stride(1) == 1 and ld >= k and ld % 8 == 0 and v.data_ptr() % 16 == 0:
            return v, ld
    return x.reshape(-1, k).contiguous(), k


def accumulate(x, score, counts, lamda=1.0, workspace=None):
    """One batch of the calibration rule, added to a key's state in place (include/micromix_calib.h, mm_calib_accumulate): x bf16 or
    fp16 [..., K] on the device, seen as rows; score fp32 [K] takes the maximum with this batch's mean |x| per channel (NaN from
    either side stays), counts int64 [2] gains the elements below the rows' p4 and p6 thresholds (reorder_indices.py:103-107).  All
    zero is the empty state.  K a multiple of 128 up to 32768, at most 2^20 rows; no rows: nothing happens.  A view whose first
    element or row stride is not at a multiple of 16 bytes is copied to a contiguous tensor first, nothing else is.  workspace: a
    contiguous device tensor of `accumulate_workspace_bytes(rows, K)` bytes, uninitialised, allocated when not given.  Runs on the
    current stream without a host synchronisation; the same inputs give the same bits on every run."""
    lib = _lib_with(*_CALIB)
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    if x.dtype not in _DTYPES:
        raise TypeError(f"x must be torch.bfloat16 or torch.float16, got {x.dtype}")
    if not x.is_cuda:
        raise RuntimeError("x must be a device tensor (HIP); the MicroMix ops have no CPU path")
    if x.dim() < 1 or x.shape[-1] < 1:
        raise RuntimeError("x must be [..., K] with K >= 1")
    lamda, dev, k = _lamda(lamda), x.device, x.shape[-1]
    score = _tensor(score, "score", torch.float32, dev, (k,), "fp32 {0}, got {1}")
    counts = _tensor(counts, "counts", torch.int64, dev, (2,), "int64 {0}, got {1}")
    x, ld = _rows(x.detach())
    rows = x.shape[0]
    if rows == 0:
        return
    need = accumulate_workspace_bytes(rows, k)
    if not need:
        _lib.check(_lib.MM_ERR_UNSUPPORTED, f"calib.accumulate (rows = {rows}, K = {k}: K a multiple of 128 in [128, 32768], rows <= 2^20)")
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
    elif (not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or workspace.device != dev or not workspace.is_contiguous()
          or workspace.numel() * workspace.element_size() < need):
        raise RuntimeError(f"workspace must be a contiguous device tensor of at least {need} bytes on {dev}")
    _launch("calib.accumulate", dev, lib.mm_calib_accumulate, _ptr(x), _DTYPES[x.dtype], rows, k, ld, lamda, _ptr(score), _ptr(counts),
            _ptr(workspace), workspace.numel() * workspace.element_size(), _stream_ptr(dev))


def accumulate_workspace_bytes(rows, k):
    """bytes of workspace `accumulate` needs for x [rows, K]; 0 for sizes it refuses and for no rows"""
    return int(_lib_with(*_CALIB).mm_calib_workspace_bytes(int(rows), int(k)))


class Calibrator:
    """The calibration statistics of a model, key by key: `hook` a model (or `observe` activations yourself), run the calibration
    texts through it, then `finish()` -- the one readback -- for the dicts `save_calibration` takes.  Per key the device holds a score
    fp32 [K] and two counts; nothing grows with the number of tokens seen."""

    def __init__(self, lamda=1.0):
        self.lamda = _lamda(lamda)
        self._state = {}            # key -> [score fp32 [K], counts int64 [2], numel]
        self._handles = []

    def observe(self, key, x):
        """one forward pass's input of the layer `key`: x bf16 / fp16 [..., K] on the device, as `accumulate` takes it"""
        if not isinstance(x, torch.Tensor) or x.dim() < 1:
            raise TypeError(f"{key}: x must be a torch.Tensor [..., K]")
        k = x.shape[-1]
        st = self._state.get(key)
        if st is None:
            st = self._state[key] = [torch.zeros(k, dtype=torch.float32, device=x.device), torch.zeros(2, dtype=torch.int64, device=x.device), 0]
        elif st[0].numel() != k:
            raise RuntimeError(f"{key}: K = {k}, seen with K = {st[0].numel()} before")
        accumulate(x, st[0], st[1], self.lamda)
        st[2] += x.numel()

    def hook(self, module, prefix=""):
        """a forward hook on every nn.Linear below `module` that observes the layer's first positional input under the key
        prefix + name + ".input" (reorder_indices.py:54-78; the reference hooks `model.model`, so that the keys start at "layers.");
        returns the handles, which `remove` takes off again"""
        handles = []
        for name, m in module.named_modules():
            if isinstance(m, torch.nn.Linear):
                handles.append(m.register_forward_hook(lambda _m, args, _out, key=prefix + name + ".input": self.observe(key, args[0])))
        self._handles += handles
        return handles

    def remove(self):
        for h in self._handles:
            h.remove()
        self._handles = []

    def keys(self):
        return list(self._state)

    def stats(self, key):
        """(score fp32 [K] where it lies, count4, count6, numel): the key's state, the counts read back as Python integers"""
        score, counts, numel = self._state[key]
        c4, c6 = counts.tolist()
        return score, c4, c6, numel

    def set_stats(self, key, score, count4, count6, numel):
        """put a key's state back (`stats`' values, from a calibration run that was interrupted or split over several processes)"""
        score = score.detach().to(torch.float32).clone()
        self._state[key] = [score, torch.tensor([int(count4), int(count6)], dtype=torch.int64, device=score.device), int(numel)]

    def finish(self, report=False):
        """-> (reorder_index, p6_nums, p8_nums), validated, for `save_calibration`; with report=True also {key: average bits} (:112).
        reorder_index[key]: the stable ascending argsort of the score (:66; the reference's sort is unstable, so any order inside a
        tie agrees with it).  The ratios are the reference's fp32 tensor arithmetic on the integer counts (:106-110), then the two
        clamps of `split_from_activations`.  A key that saw no element is left out."""
        reorder_index, p6_nums, p8_nums, bits = {}, {}, {}, {}
        for key, (score, counts, numel) in self._state.items():
            if numel == 0:
                continue
            k = score.numel()
            c4, c6 = counts.cpu().tolist()
            p4_ratio = torch.tensor(c4) / numel
            p6_ratio = torch.tensor(c6) / numel - p4_ratio
            p8_ratio = 1 - p4_ratio - p6_ratio
            p6 = math.ceil(k * p6_ratio / 128) * 128
            p8 = math.ceil(k * p8_ratio / 128) * 128
            p6 = max(0, min(p6, k))
            p8 = max(0, min(p8, k - p6))
            reorder_index[key] = torch.sort(score.cpu(), stable=True).indices
            p6_nums[key], p8_nums[key] = p6, p8
            bits[key] = float(4 * p4_ratio + 6 * p6_ratio + 8 * p8_ratio)
        validate(reorder_index, p6_nums, p8_nums)
        return (reorder_index, p6_nums, p8_nums, bits) if report else (reorder_index, p6_nums, p8_nums)
