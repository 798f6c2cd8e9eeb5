"""Sampling on the device, on the MI355X: mixedgemm.sample_rows against the torch chain it replaces.

    python tools/time_sample.py [out.txt]            (default: profiles/time_sample.txt)

Llama-3's vocabulary (128 256), 1, 21, 64 and 64 x 21 rows of Gaussian bf16 logits (standard deviation 3), temperature 0.8, and four
requests: no filter, top-k = 50, top-p = 0.9, all three (top-k 50, top-p 0.9, min-p 0.02).  Per request and size, in one alternation:
  ours     mixedgemm.sample_rows with per-row device arrays (u drawn before, outside the timed graph, as a caller's torch.rand)
  torch    softmax, sort, cumsum, mask, draw, gather in torch on the same logits (no filter: softmax, cumsum and the draw alone).  The
           draw is the inverse CDF at the same u (cumsum, compare, argmax), not torch.multinomial: the first run of this tool, with
           torch.multinomial inside the captured graph, ended in a GPU memory fault on the first replay (torch 2.10 / ROCm 7.0; one
           observation, supposed cause), so the chain here holds only operators that replay.  It costs the chain one cumsum where
           multinomial runs an exponential_ and a division
  floor    mixedgemm.argmax_rows on the same logits: one sweep over the row, which sample_rows runs first
The method is tools/time_verify.py's: each of the ITERS calls of a hipGraph reads another buffer of a pool, so that a call does not find
the logits of the call before it in the caches; every time is the median (min .. max) over REPEATS replays, taken in alternation, by
device events, divided by ITERS.  Nothing here is a gate.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from micromix_amd import mixedgemm  # noqa: E402
from time_verify import ITERS, REPEATS, VOCAB, alternate, report  # noqa: E402

TEMPERATURE, TOP_K, TOP_P, MIN_P = 0.8, 50, 0.9, 0.02
REQUESTS = {"no filter": (None, None, None), "top-k 50": (TOP_K, None, None), "top-p 0.9": (None, TOP_P, None),
            "top-k 50, top-p 0.9, min-p 0.02": (TOP_K, TOP_P, MIN_P)}
# sweeps over a row (argmax, level-1 histogram, level-2 histograms, kept mass; the draw reads one part of 16 KiB) and launches
SWEEPS = {"no filter": ("2", 4), "top-k 50": ("4", 10), "top-p 0.9": ("4", 10),
          "top-k 50, top-p 0.9, min-p 0.02": ("4 (5 when top-p's level-1 bin lies above top-k's)", 10)}
# registers and LDS of the four kernels as the compiler reports them for gfx950 (-save-temps; the build fails on scratch)
RESOURCES = "hist 32 VGPR / 3 072 B LDS, finish 22 / 3 096, mass 38 / 32, draw 109 / 2 048; no scratch"


def torch_chain(x, u, k, p, q, out):
    """the draw is the inverse CDF at the caller's u, as ours: torch.multinomial is kept out of the captured graph (module docstring)"""
    probs = torch.softmax(x.float() / TEMPERATURE, dim=-1)
    if k is None and p is None and q is None:
        cum = probs.cumsum(-1)
        out.copy_((cum > u[:, None] * cum[:, -1:]).int().argmax(-1))
        return
    sp, si = torch.sort(probs, dim=-1, descending=True)
    keep = torch.ones_like(sp, dtype=torch.bool)
    if k is not None:
        keep[:, k:] = False
    if p is not None:
        keep &= (sp.cumsum(-1) - sp) < p * (sp[:, :k].sum(-1, keepdim=True) if k is not None else 1.0)
    if q is not None:
        keep &= sp >= q * sp[:, :1]
    cum = (sp * keep).cumsum(-1)
    pick = (cum > u[:, None] * cum[:, -1:]).int().argmax(-1, keepdim=True)
    out.copy_(si.gather(1, pick).squeeze(1))


def case(rows, name, dev, gen):
    k, p, q = REQUESTS[name]
    nbytes = rows * VOCAB * 2
    pool = min(ITERS, max(2, -(-640 * 2 ** 20 // nbytes)))
    logits = [(torch.randn((rows, VOCAB), generator=gen, device=dev) * 3.0).to(torch.bfloat16) for _ in range(pool)]
    full = lambda v, dt: None if v is None else torch.full((rows,), v, dtype=dt, device=dev)
    par = dict(temperature=full(TEMPERATURE, torch.float32), top_k=full(k, torch.int32), top_p=full(p, torch.float32),
               min_p=full(q, torch.float32))
    u = torch.rand((rows,), generator=gen, device=dev)
    ours_out, arg_out = (torch.empty((rows,), dtype=torch.int32, device=dev) for _ in range(2))
    torch_out = torch.empty((rows,), dtype=torch.int64, device=dev)
    ws = torch.empty((mixedgemm.sample_rows_workspace_bytes(rows, VOCAB),), dtype=torch.uint8, device=dev)
    aws = torch.empty((max(mixedgemm.argmax_rows_workspace_bytes(rows, VOCAB), 16),), dtype=torch.uint8, device=dev)
    a = mixedgemm.sample_rows(logits[0], u, out=ours_out, workspace=ws, **par).clone()
    same = torch.equal(a, mixedgemm.sample_rows(logits[0], u, workspace=ws, **par))
    res = alternate({"mixedgemm.sample_rows": lambda i: mixedgemm.sample_rows(logits[i % pool], u, out=ours_out, workspace=ws, **par),
                     "torch softmax/sort/cumsum/mask/draw": lambda i: torch_chain(logits[i % pool], u, k, p, q, torch_out),
                     "mixedgemm.argmax_rows (floor)": lambda i: mixedgemm.argmax_rows(logits[i % pool], out=arg_out, workspace=aws)})
    return res, same, pool, nbytes, ws.numel()


def main():
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = [f"{REPEATS} replays in alternation of a hipGraph of {ITERS} calls each; us per call: median (min .. max); vocab {VOCAB}, "
             f"temperature {TEMPERATURE}", f"kernels: {RESOURCES}"]
    rows_out = []
    for nrows in (1, 21, 64, 64 * 21):
        for name in REQUESTS:
            res, same, pool, nbytes, ws_bytes = case(nrows, name, dev, gen)
            title = f"{nrows:4} x {VOCAB} ({nbytes / 2 ** 20:.1f} MB), {name}"
            report(lines, rows_out, title, res, logit_rows=nrows, request=name, bit_equal_twice=same, pool=pool, workspace_bytes=ws_bytes,
                   sweeps=SWEEPS[name][0], launches=SWEEPS[name][1])
            med = {n: float(np.median(v)) for n, v in res.items()}
            ours, chain, floor = (med[n] for n in res)
            verdict = "SLOWER than torch" if ours > chain else "faster than torch"
            lines.append(f"     -> {ours / chain:5.2f} x the torch chain ({verdict}), {ours / floor:5.2f} x argmax_rows; {SWEEPS[name][0]} sweeps, "
                         f"{SWEEPS[name][1]} launches; bit-equal twice: {same}; pool of {pool} buffers; workspace {ws_bytes / 2 ** 20:.1f} MB")
            torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    print(json.dumps(rows_out))
    default = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "time_sample.txt")
    with open(sys.argv[1] if len(sys.argv) > 1 else default, "w") as fh:
        fh.write(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}\n{text}\n{json.dumps(rows_out)}\n")


if __name__ == "__main__":
    main()
