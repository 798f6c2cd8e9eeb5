"""Token log-probabilities on the device, on the MI355X: mixedgemm.logprob_rows against the torch chains it replaces.

    python tools/time_logprob.py [out.txt]            (default: profiles/time_logprob.txt)

Llama-3's vocabulary (128 256), 1, 21, 64 and 2 047 rows (the reference's perplexity window) of Gaussian bf16 logits (standard
deviation 3) with a target per row, top_n = 0 and 20.  Per size, in one alternation:
  ours           mixedgemm.logprob_rows(x, y, top_n=...): logprob, rank and lse, with top_n = 20 top_idx and top_logprob too
  floor          mixedgemm.argmax_rows on the same logits: one sweep over the rows, which logprob_rows runs first; two sweeps is the
                 design's expectation at top_n = 0
  gather         torch.log_softmax(x.float(), -1).gather(1, y): the chain behind lm-eval style scoring
  ce fp32        F.cross_entropy(x.float(), y): the loss with the upcast
  ce bf16        F.cross_entropy(x, y): what the reference's eval_ppl runs, the loss rounded to bf16
  topk           top_n = 20 only: torch.topk(x, 20) alone, and the gather chain followed by topk(20) of the log-probabilities
Each row of the table also gives ours as a fraction of 8 TB/s on the logits' bytes read once.  The method is tools/time_verify.py's:
each of the ITERS calls of a hipGraph reads another buffer of a pool, so that a call does not find the logits of the call before it in
the caches; every time is the median (min .. max) over REPEATS replays, taken in alternation, by device events, divided by ITERS.
Nothing here is a gate.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from micromix_amd import mixedgemm  # noqa: E402
from time_verify import ITERS, PEAK, REPEATS, VOCAB, alternate, report  # noqa: E402

TOP = 20


def case(rows, top_n, dev, gen):
    nbytes = rows * VOCAB * 2
    pool = min(ITERS, max(2, -(-640 * 2 ** 20 // nbytes)))
    logits = [(torch.randn((rows, VOCAB), generator=gen, device=dev) * 3.0).to(torch.bfloat16) for _ in range(pool)]
    y = torch.randint(0, VOCAB, (rows,), generator=gen, device=dev)
    y32 = y.to(torch.int32)
    arg_out = torch.empty((rows,), dtype=torch.int32, device=dev)
    ws = torch.empty((mixedgemm.logprob_rows_workspace_bytes(rows, VOCAB, top_n),), dtype=torch.uint8, device=dev)
    aws = torch.empty((max(mixedgemm.argmax_rows_workspace_bytes(rows, VOCAB), 16),), dtype=torch.uint8, device=dev)
    a = mixedgemm.logprob_rows(logits[0], y32, top_n=top_n, workspace=ws)
    b = mixedgemm.logprob_rows(logits[0], y32, top_n=top_n, workspace=ws)
    same = all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, b) if p is not None)
    ref = torch.log_softmax(logits[0].float(), -1).gather(1, y[:, None]).squeeze(1)
    err = float((a.logprob - ref).abs().max())
    cases = {"mixedgemm.logprob_rows": lambda i: mixedgemm.logprob_rows(logits[i % pool], y32, top_n=top_n, workspace=ws),
             "mixedgemm.argmax_rows (floor)": lambda i: mixedgemm.argmax_rows(logits[i % pool], out=arg_out, workspace=aws),
             "torch log_softmax(x.float()).gather": lambda i: torch.log_softmax(logits[i % pool].float(), -1).gather(1, y[:, None]),
             "torch F.cross_entropy(x.float(), y)": lambda i: F.cross_entropy(logits[i % pool].float(), y),
             "torch F.cross_entropy(x, y) in bf16": lambda i: F.cross_entropy(logits[i % pool], y)}
    if top_n:
        cases["torch.topk(x, 20)"] = lambda i: torch.topk(logits[i % pool], top_n, dim=-1)

        def gather_and_topk(i):
            lp = torch.log_softmax(logits[i % pool].float(), -1)
            return lp.gather(1, y[:, None]), torch.topk(lp, top_n, dim=-1)
        cases["torch log_softmax.gather + topk(20)"] = gather_and_topk
    return alternate(cases), same, err, pool, nbytes, ws.numel()


def main():
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = [f"{REPEATS} replays in alternation of a hipGraph of {ITERS} calls each; us per call: median (min .. max); vocab {VOCAB}"]
    rows_out = []
    for nrows in (1, 21, 64, 2047):
        for top_n in (0, TOP):
            res, same, err, pool, nbytes, ws_bytes = case(nrows, top_n, dev, gen)
            title = f"{nrows:4} x {VOCAB} ({nbytes / 2 ** 20:.1f} MB), top_n {top_n}"
            report(lines, rows_out, title, res, logit_rows=nrows, top_n=top_n, bit_equal_twice=same, pool=pool, workspace_bytes=ws_bytes)
            med = {n: float(np.median(v)) for n, v in res.items()}
            ours, floor = med["mixedgemm.logprob_rows"], med["mixedgemm.argmax_rows (floor)"]
            chain = med["torch log_softmax.gather + topk(20)" if top_n else "torch log_softmax(x.float()).gather"]
            bf16 = med["torch F.cross_entropy(x, y) in bf16"]
            verdict = "SLOWER than torch" if ours > chain else "faster than torch"
            lines.append(f"     -> {ours / floor:5.2f} x argmax_rows, {ours / chain:5.2f} x the fp32 torch chain ({verdict}), {ours / bf16:5.2f} x the "
                         f"bf16 loss; {nbytes / (ours * 1e-6) / PEAK:6.1%} of 8 TB/s on the logits; bit-equal twice: {same}; largest "
                         f"|logprob - torch fp32| {err:.2e}; pool of {pool} buffers; workspace {ws_bytes / 2 ** 10:.1f} KiB")
            torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    print(json.dumps(rows_out))
    default = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "time_logprob.txt")
    with open(sys.argv[1] if len(sys.argv) > 1 else default, "w") as fh:
        fh.write(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}\n{text}\n{json.dumps(rows_out)}\n")


if __name__ == "__main__":
    main()
