"""MicroMix for AMD Instinct MI355X: `mixedgemm` (the ops), `qlinear` (layers), `kvcache`, `moe` (the sparse MoE block), `tp`."""


def __getattr__(name):
    # resolved on first use, so that `python -m micromix_amd.build` and the ctypes loader do not import torch
    if name == "SparseMoEBlock":
        from .moe import SparseMoEBlock
        return SparseMoEBlock
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
