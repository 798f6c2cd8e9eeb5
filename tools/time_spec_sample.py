"""Speculative sampling on the device, on the MI355X: mixedgemm.spec_sample_rows against what the step costs today and against the torch
chain that implements the same rule.

    python tools/time_spec_sample.py [out.txt]            (default: profiles/time_spec_sample.txt)

Llama-3's vocabulary (128 256), 1, 21, 64 and 64 x 21 rows of Gaussian bf16 target logits (standard deviation 3), the draft logits the
target's plus Gaussian noise of standard deviation 0.75, every candidate drawn from its draft row by mixedgemm.sample_rows under the
request's parameters, temperature 0.8.  Per size, in one alternation:
  (a) spec     mixedgemm.spec_sample_rows with draft_logits: temperature only, and with top-k 50, top-p 0.9, min-p 0.02
  (b) one-hot  mixedgemm.spec_sample_rows with draft_logits=None (temperature only)
  (c) floor    mixedgemm.sample_rows on the same target rows, temperature only and with all filters: the step's cost today
  (d) torch    two fp32 softmaxes, the ratio test at the same u_accept, the clamped difference, a cumsum and the inverse-CDF draw at the
               same u_resample (temperature only; no torch.multinomial inside a captured graph: tools/time_sample.py says why)
The method is tools/time_verify.py's: each of the ITERS calls of a hipGraph reads another pair of buffers of a pool, so that a call does
not find the logits of the call before it in the caches; every time is the median (min .. max) over REPEATS replays, taken in
alternation, by device events, divided by ITERS.  Nothing here is a gate.
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

TEMPERATURE, TOP_K, TOP_P, MIN_P, NOISE = 0.8, 50, 0.9, 0.02, 0.75
# registers and LDS of the three kernels as the compiler reports them for gfx950 (-save-temps; the build fails on scratch)
RESOURCES = "mass 38 VGPR / 32 B LDS, residual 40 / 64, draw 46 / 4 104; no scratch; the argmax is verify.hip's, the select sample.hip's"


def torch_chain(x, d, cand, ua, ur, out):
    p, q = torch.softmax(x.float() / TEMPERATURE, dim=-1), torch.softmax(d.float() / TEMPERATURE, dim=-1)
    px, qx = p.gather(1, cand[:, None]).squeeze(1), q.gather(1, cand[:, None]).squeeze(1)
    cum = (p - q).clamp_(min=0).cumsum(-1)
    pick = (cum > ur[:, None] * cum[:, -1:]).int().argmax(-1)
    out.copy_(torch.where(ua * qx < px, cand, pick))


def case(rows, dev, gen):
    nbytes = rows * VOCAB * 2
    pool = min(ITERS, max(2, -(-320 * 2 ** 20 // nbytes)))
    logits = [(torch.randn((rows, VOCAB), generator=gen, device=dev) * 3.0).to(torch.bfloat16) for _ in range(pool)]
    drafts = [(x.float() + torch.randn((rows, VOCAB), generator=gen, device=dev) * NOISE).to(torch.bfloat16) for x in logits]
    full = lambda v, dt: torch.full((rows,), v, dtype=dt, device=dev)
    temp = dict(temperature=full(TEMPERATURE, torch.float32))
    filt = dict(temp, top_k=full(TOP_K, torch.int32), top_p=full(TOP_P, torch.float32), min_p=full(MIN_P, torch.float32))
    ua, ur, ud = (torch.rand((rows,), generator=gen, device=dev) for _ in range(3))
    pars = {"temperature": temp, "all filters": filt}
    cands = {name: [mixedgemm.sample_rows(d, ud, **par) for d in drafts] for name, par in pars.items()}
    cands64 = [c.long() for c in cands["temperature"]]
    out, acc, plain = (torch.empty((rows,), dtype=torch.int32, device=dev) for _ in range(3))
    torch_out = torch.empty((rows,), dtype=torch.int64, device=dev)
    ws = torch.empty((mixedgemm.spec_sample_rows_workspace_bytes(rows, VOCAB),), dtype=torch.uint8, device=dev)
    sws = torch.empty((mixedgemm.sample_rows_workspace_bytes(rows, VOCAB),), dtype=torch.uint8, device=dev)

    def spec(i, name, draft=True):
        return mixedgemm.spec_sample_rows(logits[i % pool], drafts[i % pool] if draft else None, cands[name][i % pool], ua, ur, out=out,
                                          accepted=acc, workspace=ws, **pars[name])

    first = [t.clone() for t in spec(0, "all filters")]
    same = all(torch.equal(a, b) for a, b in zip(first, spec(0, "all filters")))
    rates = {}
    for label, name, draft in (("temperature", "temperature", True), ("all filters", "all filters", True), ("one-hot", "temperature", False)):
        rates[label] = float((spec(0, name, draft)[1] == 1).float().mean())
    torch_chain(logits[0], drafts[0], cands64[0], ua, ur, torch_out)
    rates["torch"] = float((torch_out == cands64[0]).float().mean())
    res = alternate({"(a) spec_sample_rows, temperature": lambda i: spec(i, "temperature"),
                     "(a) spec_sample_rows, all filters": lambda i: spec(i, "all filters"),
                     "(b) spec_sample_rows, one-hot": lambda i: spec(i, "temperature", False),
                     "(c) sample_rows, temperature": lambda i: mixedgemm.sample_rows(logits[i % pool], ur, out=plain, workspace=sws, **temp),
                     "(c) sample_rows, all filters": lambda i: mixedgemm.sample_rows(logits[i % pool], ur, out=plain, workspace=sws, **filt),
                     "(d) torch softmax x2/ratio/clamp/cumsum/draw": lambda i: torch_chain(logits[i % pool], drafts[i % pool], cands64[i % pool], ua, ur,
                                                                                           torch_out)})
    return res, same, rates, pool, nbytes, ws.numel()


def main():
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = [f"{REPEATS} replays in alternation of a hipGraph of {ITERS} calls each; us per call: median (min .. max); vocab {VOCAB}, "
             f"temperature {TEMPERATURE}, draft = target + N(0, {NOISE}^2)", f"kernels: {RESOURCES}"]
    rows_out = []
    for nrows in (1, 21, 64, 64 * 21):
        res, same, rates, pool, nbytes, ws_bytes = case(nrows, dev, gen)
        title = f"{nrows:4} x {VOCAB} (2 x {nbytes / 2 ** 20:.1f} MB)"
        report(lines, rows_out, title, res, logit_rows=nrows, bit_equal_twice=same, pool=pool, workspace_bytes=ws_bytes, accepted=rates)
        med = {n: float(np.median(v)) for n, v in res.items()}
        spread = {n: (min(v), max(v)) for n, v in res.items()}
        a_t, a_f, b, c_t, c_f, d = (med[n] for n in res)
        lo_hi = lambda x, y: f"{spread[x][0] / spread[y][1]:.2f} .. {spread[x][1] / spread[y][0]:.2f}"
        names = list(res)
        verdict = "SLOWER than torch" if a_t > d else "faster than torch"
        lines.append(f"     -> (a)/(c) temperature {a_t / c_t:5.2f} ({lo_hi(names[0], names[3])}), all filters {a_f / c_f:5.2f} "
                     f"({lo_hi(names[1], names[4])}); (b)/(c) {b / c_t:5.2f}; (a)/(d) {a_t / d:5.2f} ({lo_hi(names[0], names[5])}, {verdict}); "
                     f"accepted: {', '.join(f'{n} {r:.2f}' for n, r in rates.items())}; bit-equal twice: {same}; pool of {pool} pairs; "
                     f"workspace {ws_bytes / 2 ** 20:.1f} MB")
        del res
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    print(json.dumps(rows_out))
    default = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "time_spec_sample.txt")
    with open(sys.argv[1] if len(sys.argv) > 1 else default, "w") as fh:
        fh.write(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}\n{text}\n{json.dumps(rows_out)}\n")


if __name__ == "__main__":
    main()
