"""The token half of a decode step on the device (mixedgemm.ngram_draft, mixedgemm.token_step), on the MI355X.

    python tools/time_token_step.py [out.txt]            (default: profiles/time_token_step.txt)

(a) ngram_draft for 1 and 64 sequences with histories of N = 1 024, 32 768 and 131 072 tokens (ld_tok = N + 64), max_n = 4 and 16,
    min_n = 2, a chain of 6 nodes a sequence.  The histories are uniform over a vocabulary of 128 256 with the last 8 tokens planted once
    in the middle, so every sequence has a match and few positions pass the filter; one more row takes histories over an alphabet of 3,
    where a third of the positions pass it and are extended.  us per call inside a hipGraph of ITERS calls, device events, median
    (min .. max) over REPEATS replays, and the history's bytes (4 N a sequence) over that time as a fraction of 8 TB/s.
(b) the same rule as a torch chain on the device in the same kind of graph: unfold the history into windows of max_n, compare with the
    suffix, cumprod over the reversed window for the match length, max over m << 24 | e, gather the continuation.  It takes N as a host
    number and leaves out the first max_n - 1 end positions; its draft is checked against ours.
(c) the host path by a host clock: the histories to the host, a numpy search (candidates by h == h[N - 1], then one vector compare per
    n-gram position), the draft uploaded, a synchronise: what a loop without the op does every step.
(d) token_step for 1 and 64 sequences, a chain of 6 with 3 kept, two stop tokens a sequence: us per call in a hipGraph.
Nothing here is a gate.
"""
from __future__ import annotations

import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from micromix_amd import mixedgemm  # noqa: E402

ITERS, WARM, REPEATS = 20, 2, 9
VOCAB, NODES, MIN_N, SLACK = 128256, 6, 2, 64


def histories(B, N, alphabet, dev):
    rng = np.random.default_rng(N + B)
    h = rng.integers(0, alphabet, (B, N + SLACK)).astype(np.int32)
    if alphabet > 3:
        h[:, N // 2:N // 2 + 8] = h[:, N - 8:N]                  # the match: 8 tokens, found once
    return torch.from_numpy(h).to(dev)


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


def torch_draft(tokens, N, max_n, out):
    """the rule as a torch chain, N a host number, end positions max_n - 1 .. N - 2"""
    h = tokens[:, :N]
    windows = h[:, :N - 1].unfold(1, max_n, 1)                   # [B, N - max_n, max_n]: window j ends at e = j + max_n - 1
    eq = windows == h[:, None, N - max_n:]
    m = eq.flip(-1).to(torch.int32).cumprod(-1).sum(-1)
    e = torch.arange(max_n - 1, N - 1, device=tokens.device, dtype=torch.int32)
    key = (m << 24 | e).amax(-1)
    hit, at = (key >> 24) >= MIN_N, (key & 0xFFFFFF).to(torch.int64)
    period = (N - 1 - at).clamp_(min=1)
    idx = at[:, None] + 1 + torch.arange(NODES - 1, device=tokens.device)[None, :] % period[:, None]
    last = h[:, N - 1:N]
    out[:, 0:1] = last
    out[:, 1:] = torch.where(hit[:, None], torch.gather(h, 1, idx.clamp_(max=N - 1)), last)
    return out


def host_draft(tokens, N, max_n, dev):
    """history down, numpy search, draft up"""
    h = tokens[:, :N].cpu().numpy()
    out = np.empty((h.shape[0], NODES), dtype=np.int32)
    for b, row in enumerate(h):
        cand = np.flatnonzero(row[:N - 1] == row[N - 1])
        m, alive = np.ones(len(cand), dtype=np.int64), np.ones(len(cand), dtype=bool)
        for i in range(1, max_n):
            alive &= cand - i >= 0
            alive[alive] = row[cand[alive] - i] == row[N - 1 - i]
            m += alive
        out[b] = row[N - 1]
        if len(cand):
            best = int(np.argmax(m << 24 | cand))
            if m[best] >= MIN_N:
                e = int(cand[best])
                out[b, 1:] = row[e + 1 + np.arange(NODES - 1) % (N - 1 - e)]
    return torch.from_numpy(out).to(dev)


def host_us(call):
    us = []
    for rep in range(REPEATS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        if rep:
            us.append((time.perf_counter() - t0) * 1e6)
    return us


def main():
    dev = torch.device("cuda:0")
    lines = [f"us per call: median (min .. max) over {REPEATS}; in a hipGraph of {ITERS} calls unless it says host clock; chains of {NODES} nodes, min_n {MIN_N}"]
    rows = []

    def report(case, name, us, extra=""):
        med = float(np.median(us))
        rows.append(dict(case=case, call=name, median_us=round(med, 2), min_us=round(min(us), 2), max_us=round(max(us), 2)))
        lines.append(f"{case:48} {name:28} {med:10.2f} ({min(us):.2f} .. {max(us):.2f}){extra}")
        return med

    def draft_case(B, N, max_n, alphabet, baselines=True):
        tokens = histories(B, N, alphabet, dev)
        total = torch.full((B,), N, dtype=torch.int32, device=dev)
        indptr = torch.arange(0, (B + 1) * NODES, NODES, dtype=torch.int32, device=dev)
        T = B * NODES
        z = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
        outs = dict(draft_tok=z(T), root_tok=z(B), cand_tok=z(T), match_len=z(B), row_seq=z(T), row_total_len=z(T))
        need = mixedgemm.ngram_draft_workspace_bytes(B, N + SLACK)
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        case = f"{B:2} x {N:6} tokens, max_n {max_n:2}" + ("" if alphabet > 3 else ", alphabet of 3")
        ours = report(case, "ngram_draft", graph_us(lambda: mixedgemm.ngram_draft(tokens, total, indptr, T, min_n=MIN_N, max_n=max_n, workspace=ws if need else None, **outs)))
        lines[-1] += f"   {B * N * 4 / (ours * 1e-6) / 8e12:.4f} of 8 TB/s on the history"
        if not baselines:
            return
        mine = outs["draft_tok"].view(B, NODES).clone()
        assert int(outs["match_len"].min()) >= min(8, max_n), "the planted match was not found"
        out = torch.zeros((B, NODES), dtype=torch.int32, device=dev)
        t_us = report(case, "torch chain", graph_us(lambda: torch_draft(tokens, N, max_n, out)))
        assert torch.equal(out, mine), "the torch chain drafts something else"
        h_us = report(case, "host path, host clock", host_us(lambda: host_draft(tokens, N, max_n, dev)))
        assert torch.equal(host_draft(tokens, N, max_n, dev), mine), "the host path drafts something else"
        lines.append(f"{'':48} ours / torch {ours / t_us:.3f}, ours / host {ours / h_us:.4f}")
        del tokens, out
        torch.cuda.empty_cache()

    for B in (1, 64):
        for N in (1024, 32768, 131072):
            for max_n in (4, 16):
                draft_case(B, N, max_n, VOCAB)
    draft_case(64, 131072, 16, 3, baselines=False)
    draft_case(1, 131072, 16, 3, baselines=False)

    for B in (1, 64):
        ld, n, k = 4096, NODES, 3
        tokens = torch.zeros((B, ld), dtype=torch.int32, device=dev)
        total, finished = torch.full((B,), 16, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        result = torch.full((B, 66), -1, dtype=torch.int32, device=dev)
        result[:, 0], result[:, 1] = k, 7
        result[:, 2:2 + k] = torch.arange(k, dtype=torch.int32, device=dev)
        target = torch.arange(B * n, dtype=torch.int32, device=dev) % 1000 + 10
        qo = torch.arange(0, (B + 1) * n, n, dtype=torch.int32, device=dev)
        root, most = torch.full((B,), 5, dtype=torch.int32, device=dev), torch.full((B,), ld, dtype=torch.int32, device=dev)
        stops, emitted = torch.full((B, 2), 2, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        us = graph_us(lambda: mixedgemm.token_step(tokens, total, finished, result, target, qo, root, most, stop_tok=stops, emitted=emitted))
        assert int(finished.max()) == 0 and int(total.min()) == 16 + k * (WARM + ITERS * (REPEATS + 1)), "the steps did not all commit"
        report(f"{B:2} sequences, chain of {n}, {k} kept", "token_step", us)

    text = "\n".join(lines)
    print(text)
    print(json.dumps(rows))
    default = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "time_token_step.txt")
    with open(sys.argv[1] if len(sys.argv) > 1 else default, "w") as fh:
        fh.write(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}\n{text}\n{json.dumps(rows)}\n")


if __name__ == "__main__":
    main()
