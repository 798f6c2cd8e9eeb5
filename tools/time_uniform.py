"""Seeded uniform numbers on the device (mixedgemm.uniform_rows), on the MI355X.

    python tools/time_uniform.py [out.txt]            (default: profiles/time_uniform.txt)

(a) uniform_rows for 1, 64 and 1 344 rows (64 sequences x 21 nodes) with n = 3 and n = 16 streams, row_seq and sub given, against
    (b) torch.rand((3, rows)) -- what a caller of sample_rows / spec_sample_rows writes today -- in the same kind of graph: us per call
    inside a hipGraph of ITERS calls, device events, median (min .. max) over REPEATS replays.
(c) the sampled step uniform_rows -> spec_sample_rows against torch.rand -> spec_sample_rows on the same rows (vocab 128 256, Gaussian
    bf16 logits, the one-hot form with the candidate the row's argmax or a random token, temperature 0.8): us per pair of calls.
Two calls of uniform_rows are checked to be bit-equal.  Nothing here is a gate.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from micromix_amd import mixedgemm  # noqa: E402

ITERS, WARM, REPEATS = 20, 2, 9
VOCAB, ROWS = 128256, (1, 64, 1344)


def graph_us(call):
    """us per call inside a graph of ITERS of them: REPEATS replays between device events"""
    for _ in range(WARM):
        call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(ITERS):
            call()
    g.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / ITERS)
    return us


def main():
    dev = torch.device("cuda:0")
    lines = [f"us per call: median (min .. max) over {REPEATS}; in a hipGraph of {ITERS} calls"]
    rows_out = []

    def report(case, name, us):
        med = float(np.median(us))
        rows_out.append(dict(case=case, call=name, median_us=round(med, 2), min_us=round(min(us), 2), max_us=round(max(us), 2)))
        lines.append(f"{case:40} {name:36} {med:10.2f} ({min(us):.2f} .. {max(us):.2f})")
        return med

    gen = torch.Generator(device="cpu").manual_seed(1)
    for rows in ROWS:
        batch = max(1, rows // 21)
        seed = torch.randint(-2 ** 62, 2 ** 62, (batch,), generator=gen, dtype=torch.int64).to(dev)
        sub = torch.zeros(batch, dtype=torch.int32, device=dev)
        row_seq = (torch.arange(rows, dtype=torch.int32) % batch).to(dev)
        pos = torch.randint(0, 8192, (rows,), generator=gen, dtype=torch.int32).to(dev)
        case = f"{rows:5} rows, {batch:2} sequences"
        ours = {}
        for n in (3, 16):
            out = torch.zeros((n, rows), dtype=torch.float32, device=dev)
            ours[n] = report(case, f"uniform_rows n = {n}", graph_us(lambda: mixedgemm.uniform_rows(seed, pos, n=n, sub=sub, row_seq=row_seq, out=out)))
            again = mixedgemm.uniform_rows(seed, pos, n=n, sub=sub, row_seq=row_seq)
            assert torch.equal(again, out) and float(out.max()) < 1.0 and float(out.min()) >= 0.0, "two calls differ"
        rand = report(case, "torch.rand((3, rows))", graph_us(lambda: torch.rand((3, rows), device=dev)))
        lines.append(f"{'':40} uniform_rows n = 3 / torch.rand {ours[3] / rand:.3f}")

        # the sampled step
        logits = (torch.randn((rows, VOCAB), generator=gen, dtype=torch.float32) * 3.0).to(torch.bfloat16).to(dev)
        cand = logits.argmax(-1).to(torch.int32)
        cand[::2] = torch.randint(0, VOCAB, (rows,), generator=gen, dtype=torch.int32).to(dev)[::2]
        temperature = torch.full((rows,), 0.8, dtype=torch.float32, device=dev)
        target, accepted = torch.zeros(rows, dtype=torch.int32, device=dev), torch.zeros(rows, dtype=torch.int32, device=dev)
        ws = torch.empty(max(1, mixedgemm.spec_sample_rows_workspace_bytes(rows, VOCAB)), dtype=torch.uint8, device=dev)
        u = torch.zeros((2, rows), dtype=torch.float32, device=dev)

        def seeded_step():
            mixedgemm.uniform_rows(seed, pos, n=2, sub=sub, row_seq=row_seq, out=u)
            mixedgemm.spec_sample_rows(logits, None, cand, u[0], u[1], temperature=temperature, out=target, accepted=accepted, workspace=ws)

        def rand_step():
            r = torch.rand((2, rows), device=dev)
            mixedgemm.spec_sample_rows(logits, None, cand, r[0], r[1], temperature=temperature, out=target, accepted=accepted, workspace=ws)

        a = report(case, "uniform_rows -> spec_sample_rows", graph_us(seeded_step))
        first = target.clone()
        seeded_step()
        assert torch.equal(first, target), "the seeded step is not a function of its inputs"
        b = report(case, "torch.rand -> spec_sample_rows", graph_us(rand_step))
        lines.append(f"{'':40} seeded step / torch.rand step {a / b:.3f}")
        del logits
        torch.cuda.empty_cache()

    text = "\n".join(lines)
    print(text)
    print(json.dumps(rows_out))
    default = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "time_uniform.txt")
    with open(sys.argv[1] if len(sys.argv) > 1 else default, "w") as fh:
        fh.write(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}\n{text}\n{json.dumps(rows_out)}\n")


if __name__ == "__main__":
    main()
