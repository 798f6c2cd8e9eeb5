"""Logits processing on the device, on the MI355X: mixedgemm.process_logits against the torch chain it replaces and against a copy.

    python tools/time_logits.py [out.txt]            (default: profiles/time_logits.txt)

Llama-3's vocabulary (128 256), 1, 21, 64 and 1 344 rows of Gaussian bf16 logits (standard deviation 3), a token history of 1 024 and
of 8 192 tokens per row (a quarter of it prompt, ids uniform over the vocabulary), 16 bias entries per row and a bitmask that allows
half the tokens.  Per size, in one alternation:
  all            mixedgemm.process_logits with the three penalties, the bias list and the mask
  penalties      ... with the three penalties only
  mask           ... with the mask only (no history: its length does not matter to this line)
  torch all /    the chain a caller writes today, in fp32 on the device: counts by scatter_add into [rows, vocab], where() for the
  penalties /    repetition penalty, two elementwise passes for frequency and presence, scatter_add of the bias, the bitmask unpacked
  mask           and masked_fill, .to(bfloat16) into the same output; the parts that the line of ours leaves out are left out
  copy           out.copy_(logits): the floor on the bytes, rows x vocab x 2 read and written
Each row of the table also gives ours as a multiple of the copy and of the torch chain.  The method is tools/time_verify.py's: each of
the ITERS calls of a hipGraph reads another buffer of a pool, so that a call does not find the logits of the call before it in the
caches; every time is the median (min .. max) over REPEATS replays, taken in alternation, by device events, divided by ITERS.
Nothing here is a gate.
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

N_BIAS = 16


def torch_chain(x, out, tokens, prompt_len, total_len, theta, alpha_f, alpha_p, bias_idx, bias_val, mask, penalties, bias_and_mask):
    """the chain of today, on x bf16 [rows, vocab]; every tensor on the device, nothing read on the host"""
    rows, vocab = x.shape
    y = x.float()
    if penalties:
        pos = torch.arange(tokens.size(1), device=x.device)[None, :]
        in_all = (pos < total_len[:, None]).float()
        in_out = ((pos >= prompt_len[:, None]) & (pos < total_len[:, None])).float()
        ids = tokens.long()
        seen = torch.zeros((rows, vocab), dtype=torch.float32, device=x.device).scatter_add_(1, ids, in_all) > 0
        counts = torch.zeros((rows, vocab), dtype=torch.float32, device=x.device).scatter_add_(1, ids, in_out)
        y = torch.where(seen, torch.where(y < 0, y * theta[:, None], y / theta[:, None]), y)
        y = y - alpha_f[:, None] * counts
        y = y - alpha_p[:, None] * (counts > 0)
    if bias_and_mask:
        y = y.scatter_add(1, bias_idx.long(), bias_val)
    if mask is not None:
        shifts = torch.arange(32, device=x.device, dtype=torch.int32)
        allowed = ((mask[:, :, None] >> shifts) & 1).bool().view(rows, -1)[:, :vocab]
        y = y.masked_fill(~allowed, float("-inf"))
    out.copy_(y)
    return out


def case(rows, hist, dev, gen):
    nbytes = rows * VOCAB * 2
    pool = min(ITERS, max(2, -(-640 * 2 ** 20 // nbytes)))
    logits = [(torch.randn((rows, VOCAB), generator=gen, device=dev) * 3.0).to(torch.bfloat16) for _ in range(pool)]
    out = torch.empty((rows, VOCAB), dtype=torch.bfloat16, device=dev)
    ref = torch.empty((rows, VOCAB), dtype=torch.bfloat16, device=dev)
    tokens = torch.randint(0, VOCAB, (rows, hist), generator=gen, device=dev, dtype=torch.int32)
    prompt_len = torch.full((rows,), hist // 4, dtype=torch.int32, device=dev)
    total_len = torch.full((rows,), hist, dtype=torch.int32, device=dev)
    theta = torch.full((rows,), 1.2, dtype=torch.float32, device=dev)
    alpha_f = torch.full((rows,), 0.1, dtype=torch.float32, device=dev)
    alpha_p = torch.full((rows,), 0.5, dtype=torch.float32, device=dev)
    bias_idx = torch.stack([torch.randperm(VOCAB, generator=gen, device=dev)[:N_BIAS] for _ in range(min(rows, 8))]).to(torch.int32)
    bias_idx = bias_idx.repeat(-(-rows // bias_idx.size(0)), 1)[:rows].contiguous()                # distinct per row: scatter_add then agrees
    bias_val = torch.randn((rows, N_BIAS), generator=gen, device=dev)
    mask = torch.randint(-2 ** 31, 2 ** 31, (rows, (VOCAB + 31) // 32), generator=gen, device=dev, dtype=torch.int64).to(torch.int32)
    pen = dict(tokens=tokens, prompt_len=prompt_len, total_len=total_len, repetition_penalty=theta, frequency_penalty=alpha_f,
               presence_penalty=alpha_p)
    rest = dict(bias_idx=bias_idx, bias_val=bias_val, allowed_mask=mask)
    a = mixedgemm.process_logits(logits[0], **pen, **rest).clone()
    b = mixedgemm.process_logits(logits[0], out=out, **pen, **rest)
    same = torch.equal(a.view(torch.int16), b.view(torch.int16))
    torch_chain(logits[0], ref, tokens, prompt_len, total_len, theta, alpha_f, alpha_p, bias_idx, bias_val, mask, True, True)
    differ = int((ref.view(torch.int16) != a.view(torch.int16)).sum())             # torch's own roundings: reported, not required to be 0
    args = (tokens, prompt_len, total_len, theta, alpha_f, alpha_p, bias_idx, bias_val)
    cases = {"process_logits all": lambda i: mixedgemm.process_logits(logits[i % pool], out=out, **pen, **rest),
             "process_logits penalties": lambda i: mixedgemm.process_logits(logits[i % pool], out=out, **pen),
             "process_logits mask": lambda i: mixedgemm.process_logits(logits[i % pool], out=out, allowed_mask=mask),
             "torch all": lambda i: torch_chain(logits[i % pool], ref, *args, mask, True, True),
             "torch penalties": lambda i: torch_chain(logits[i % pool], ref, *args, None, True, False),
             "torch mask": lambda i: torch_chain(logits[i % pool], ref, *args, mask, False, False),
             "out.copy_(logits)": lambda i: out.copy_(logits[i % pool])}
    return alternate(cases), same, differ, pool, nbytes


def main():
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = [f"{REPEATS} replays in alternation of a hipGraph of {ITERS} calls each; us per call: median (min .. max); vocab {VOCAB}, "
             f"{N_BIAS} bias entries per row"]
    rows_out = []
    for nrows in (1, 21, 64, 1344):
        for hist in (1024, 8192):
            res, same, differ, pool, nbytes = case(nrows, hist, dev, gen)
            title = f"{nrows:4} x {VOCAB} ({nbytes / 2 ** 20:.1f} MB), history {hist}"
            report(lines, rows_out, title, res, logit_rows=nrows, history=hist, bit_equal_twice=same, pool=pool)
            med = {n: float(np.median(v)) for n, v in res.items()}
            copy = med["out.copy_(logits)"]
            for kind in ("all", "penalties", "mask"):
                ours, chain = med[f"process_logits {kind}"], med[f"torch {kind}"]
                verdict = "SLOWER than torch" if ours > chain else "faster than torch"
                lines.append(f"     -> {kind:9} {ours / copy:5.2f} x the copy, {ours / chain:6.3f} x the torch chain ({verdict})")
            lines.append(f"     -> bit-equal twice: {same}; elements where torch's fp32 chain rounds to another bf16: {differ} of {nrows * VOCAB}; "
                         f"pool of {pool} buffers")
            torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    print(json.dumps(rows_out))
    default = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "time_logits.txt")
    with open(sys.argv[1] if len(sys.argv) > 1 else default, "w") as fh:
        fh.write(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}\n{text}\n{json.dumps(rows_out)}\n")


if __name__ == "__main__":
    main()
