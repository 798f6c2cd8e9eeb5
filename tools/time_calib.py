"""Calibration statistics on the device, on the MI355X: calib.Calibrator.observe against a torch chain on the device that keeps the same
state, and against the reference's route (every activation copied to the host as fp32).

    python tools/time_calib.py [out.txt]            (default: profiles/time_calib.txt)

bf16 activations [2048, 4096], [2048, 14336] and [1, 4096], Gaussian with 1 % of the channels 20 times larger.  Per shape:
  observe      Calibrator.observe in a Python loop of ITERS calls between two device events: what a forward hook costs.  At these sizes
               the loop is bound by the host (argument checks, one workspace allocation and two launches per call), so also
  accumulate   calib.accumulate with a workspace passed in, the same loop; and
  graph        ITERS calls of calib.accumulate captured in one hipGraph, replayed between two events: the two kernels alone
  torch        abs, max over the row, the two thresholds, the two compares and sums, mean over the rows, maximum with the score, in
               torch on the device, updating the same state in place; as a loop and as a graph
  host         the reference's route for one call (reorder_indices.py:43-47, 103-107): x.float().cpu().abs(), the mean and its maximum,
               and the two counts of that batch on the host; host clock around a synchronise, HOST_REPEATS calls
Each of the ITERS calls reads another buffer of a pool larger than the 256 MB Infinity Cache, so that a call does not find its
activation in the caches.  Every time is the median (min .. max) over REPEATS runs taken in alternation.  The share of peak is the time
8 TB/s needs for the activation's own bytes (rows * K * 2) over the graph time.  Nothing here is a gate.
"""
from __future__ import annotations

import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from micromix_amd import calib  # noqa: E402

ITERS, WARM, REPEATS, HOST_REPEATS = 100, 3, 7, 3
SHAPES = ((2048, 4096), (2048, 14336), (1, 4096))
PEAK = 8e12                                         # bytes / s
LAMDA = 1.0


def torch_chain(x, score, counts):
    v = x.float().abs()
    m = v.max(dim=-1, keepdim=True)[0]
    counts[0] += (v < m * 448 / 6 / 1024 * LAMDA).sum()
    counts[1] += (v < m * 448 / 28 / 64 * LAMDA).sum()
    torch.maximum(score, v.mean(dim=0), out=score)


def host_route(x, state):
    v = x.view(-1, x.shape[-1]).float().detach().cpu().abs()
    mean = torch.mean(v, dim=0).float()
    state["score"] = mean if "score" not in state else torch.max(state["score"], mean)
    m = v.max(dim=-1, keepdim=True)[0]
    state["c4"] = state.get("c4", 0) + int((v < m * 448 / 6 / 1024 * LAMDA).sum())
    state["c6"] = state.get("c6", 0) + int((v < m * 448 / 28 / 64 * LAMDA).sum())


def looped(fn):
    def run():
        for i in range(ITERS):
            fn(i)
    return run


def graphed(fn):
    """a hipGraph of ITERS back-to-back calls fn(0) .. fn(ITERS - 1), warmed up on a side stream first (tools/time_verify.py)"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for i in range(WARM):
            fn(i)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(ITERS):
            fn(i)
    return g.replay


def alternate(runs):
    for run in runs.values():
        run()
    torch.cuda.synchronize()
    out = {n: [] for n in runs}
    for _ in range(REPEATS):
        for n, run in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            torch.cuda.synchronize()
            out[n].append(a.elapsed_time(b) * 1e3 / ITERS)     # us per call
    return out


def case(rows, k, dev, gen):
    nbytes = rows * k * 2
    pool = min(ITERS, max(2, -(-640 * 2 ** 20 // nbytes)))
    xs = []
    for _ in range(pool):
        x = torch.randn((rows, k), generator=gen, device=dev)
        x[:, ::100] *= 20.0
        xs.append(x.to(torch.bfloat16))
    state = lambda: (torch.zeros(k, dtype=torch.float32, device=dev), torch.zeros(2, dtype=torch.int64, device=dev))
    ws = torch.empty((calib.accumulate_workspace_bytes(rows, k),), dtype=torch.uint8, device=dev)
    cal = calib.Calibrator(LAMDA)
    (s_loop, c_loop), (s_graph, c_graph), (ts_loop, tc_loop), (ts_graph, tc_graph) = state(), state(), state(), state()
    # the two routes keep the same state, up to torch's own arithmetic on the device (its fp32 mean, and a division by a scalar that it
    # may turn into a multiplication by the reciprocal, which moves a threshold by an ulp)
    calib.accumulate(xs[0], s_loop, c_loop, LAMDA, ws)
    torch_chain(xs[0], ts_loop, tc_loop)
    same = (f"counts {c_loop.tolist()} against the torch chain's {tc_loop.tolist()}, largest relative score difference "
            f"{float(((s_loop - ts_loop).abs() / ts_loop).max()):.2e}")
    res = alternate({
        "Calibrator.observe, loop": looped(lambda i: cal.observe("k", xs[i % pool])),
        "calib.accumulate, loop": looped(lambda i: calib.accumulate(xs[i % pool], s_loop, c_loop, LAMDA, ws)),
        "calib.accumulate, graph": graphed(lambda i: calib.accumulate(xs[i % pool], s_graph, c_graph, LAMDA, ws)),
        "torch chain on the device, loop": looped(lambda i: torch_chain(xs[i % pool], ts_loop, tc_loop)),
        "torch chain on the device, graph": graphed(lambda i: torch_chain(xs[i % pool], ts_graph, tc_graph)),
    })
    host, hstate = [], {}
    for i in range(HOST_REPEATS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_route(xs[i % pool], hstate)
        host.append((time.perf_counter() - t0) * 1e6)
    res["reference route (fp32 copy to the host), one call"] = host[1:]
    return res, same, pool, nbytes, ws.numel()


def main():
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = [f"{REPEATS} runs in alternation of {ITERS} calls each (the host route: {HOST_REPEATS} single calls); us per call: median (min .. max); "
             f"bf16, lamda {LAMDA}"]
    rows_out = []
    for rows, k in SHAPES:
        res, same, pool, nbytes, ws_bytes = case(rows, k, dev, gen)
        title = f"[{rows}, {k}] ({nbytes / 2 ** 20:.2f} MB)"
        med = {n: float(np.median(v)) for n, v in res.items()}
        for name, us in res.items():
            rows_out.append(dict(case=title, call=name, median_us=round(med[name], 2), min_us=round(min(us), 2), max_us=round(max(us), 2)))
            lines.append(f"{title:28} {name:52} {med[name]:11.2f} ({min(us):.2f} .. {max(us):.2f}) us")
        floor = nbytes / PEAK * 1e6
        ours, chain = med["calib.accumulate, graph"], med["torch chain on the device, graph"]
        verdict = "SLOWER than the torch chain" if ours > chain else "faster than the torch chain"
        lines.append(f"     -> {floor:.2f} us at 8 TB/s on the activation's bytes: {floor / ours:.1%} of that rate in the graph; {ours / chain:.2f} x the torch "
                     f"chain's graph ({verdict}); in the loop {med['Calibrator.observe, loop'] / med['torch chain on the device, loop']:.2f} x the "
                     f"torch chain's loop; pool of {pool} buffers; workspace {ws_bytes / 2 ** 10:.0f} KB")
        lines.append(f"        first call: {same}")
        del res
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    print(json.dumps(rows_out))
    default = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "time_calib.txt")
    with open(sys.argv[1] if len(sys.argv) > 1 else default, "w") as fh:
        fh.write(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}\n{text}\n{json.dumps(rows_out)}\n")


if __name__ == "__main__":
    main()
