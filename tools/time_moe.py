"""The sparse MoE block on the MI355X: micromix_amd.moe.SparseMoEBlock against the per-expert loop it replaces, and its four new kernels.

    python tools/time_moe.py [out.txt]
    python tools/time_moe.py device [out.txt]     the capturable block (device-sized grouped launches), see device_main
    python tools/time_moe.py activate [out.txt]   the fused silu * mul + expert quantizer (fused_activation=True), see activate_main
    python tools/time_moe.py gate_up [out.txt]    w1 | w3, silu * mul and w2's quantizer in one launch (fused_gate_up=True), see gate_up_main

Mixtral-8x7B shapes (H 4096, I 14336, E 8, top_k 2; splits as tests/test_model_shapes_gpu.py), T = 1, 16, 128, 4096, one set of weights.
1. The block (`SparseMoEBlock.forward`: one host sync) and the reference's loop (model/qMixtralLayer.py:414-452, 502-519) written with
   this library's per-expert ops -- torch softmax / topk / one_hot / where, reorder_quantize_x, matmul, F.silu * , index_add_ -- once
   with the reference's two torch.cuda.synchronize() per expert and once without them.  Time = device events around ITERS back-to-back
   calls / ITERS, so host gaps between launches count, as they do for a model.
2. moe_route, moe_plan, moe_gather, moe_combine alone: ten calls captured in one hipGraph (no host time), replay time / 10; their sum
   as a share of the block's time; for gather and combine the bytes they move as TB/s and as a fraction of 8 TB/s.
"""
from __future__ import annotations

import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from micromix_amd import SparseMoEBlock, mixedgemm  # noqa: E402
from micromix_amd.qlinear import QLinearLayer  # noqa: E402

H, I, E, K = 4096, 14336, 8, 2
SPLIT_H, SPLIT_I = (3584, 256, 256), (12544, 1024, 768)
WARM = 3


def timed(fn, iters):
    for _ in range(WARM):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters     # us


def graph_time(fn, calls=10, iters=20):
    """us per call of `fn` when `calls` of them replay as one hipGraph"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(calls):
            fn()
    return timed(graph.replay, iters) / calls


def make_experts(dev):
    g = torch.Generator(device=dev).manual_seed(0)
    out = []
    for e in range(E):
        i1 = torch.randperm(H, generator=g, device=dev).to(torch.int16)
        i2 = torch.randperm(I, generator=g, device=dev).to(torch.int16)
        layers = []
        for n, k, split, idx in ((I, H, SPLIT_H, i1), (I, H, SPLIT_H, i1), (H, I, SPLIT_I, i2)):
            lin = torch.nn.Linear(k, n, bias=False, dtype=torch.bfloat16, device=dev)
            lin.weight.data = (torch.randn((n, k), generator=g, device=dev) * 0.02).to(torch.bfloat16)
            layers.append(QLinearLayer(lin, p8_num=split[2], p6_num=split[1], reorder_index=idx))
            del lin
        out.append(tuple(layers))
    return out


def reference_loop(x, gate_w, experts, syncs):
    mm = lambda q, l: mixedgemm.matmul(q[0], l.BN, q[1], l.BS, q[2], l.BO, q[3], l.SFBN, q[4], l.SFBS, q[5], l.SFBO)
    logits = F.linear(x, gate_w)
    rw = F.softmax(logits, dim=1, dtype=torch.float)
    rw, sel = torch.topk(rw, K, dim=-1)
    rw = (rw / rw.sum(dim=-1, keepdim=True)).to(x.dtype)
    final = torch.zeros_like(x)
    mask = F.one_hot(sel, num_classes=E).permute(2, 1, 0)
    for e, (w1, w3, w2) in enumerate(experts):
        idx, top_x = torch.where(mask[e])
        if top_x.numel() == 0:
            continue
        cur = x[None, top_x].reshape(-1, H)
        q = mixedgemm.reorder_quantize_x(cur, w1.reorder_index, w1.p4_num, w1.p6_num, w1.p8_num)
        if syncs:
            torch.cuda.synchronize()
        h = F.silu(mm(q, w1)) * mm(q, w3)
        q = mixedgemm.reorder_quantize_x(h, w2.reorder_index, w2.p4_num, w2.p6_num, w2.p8_num)
        if syncs:
            torch.cuda.synchronize()
        final.index_add_(0, top_x, mm(q, w2) * rw[top_x, idx, None])
    return final


def main():
    dev = torch.device("cuda:0")
    experts = make_experts(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    gate_w = (torch.randn((E, H), generator=g, device=dev) * 0.05).to(torch.bfloat16)
    block = SparseMoEBlock(gate_w, experts, K)
    lines, rows = [], []
    lines.append(f"{'T':>5} {'block us':>9} {'loop us':>9} {'loop + ref syncs us':>20} | {'route':>7} {'plan':>7} {'gather':>7} {'combine':>8} {'share':>6} |"
                 f" {'gather TB/s (/8)':>17} {'combine TB/s (/8)':>18}   rows per expert")
    for T in (1, 16, 128, 4096):
        x = torch.randn((T, H), generator=g, device=dev).to(torch.bfloat16)
        iters = 20 if T >= 4096 else 50
        block_us = timed(lambda: block(x), iters)
        loop_us = timed(lambda: reference_loop(x, gate_w, experts, False), iters)
        loop_sync_us = timed(lambda: reference_loop(x, gate_w, experts, True), iters)
        logits = F.linear(x, gate_w)
        ids, w = mixedgemm.moe_route(logits, K)
        off, tok, slot = mixedgemm.moe_plan(ids, E)
        xs = mixedgemm.moe_gather(x, tok)
        y = torch.randn((T * K, H), generator=g, device=dev).to(torch.bfloat16)
        out = torch.empty((T, H), dtype=torch.bfloat16, device=dev)
        us = dict(route=graph_time(lambda: mixedgemm.moe_route(logits, K, topk_ids=ids, topk_w=w)),
                  plan=graph_time(lambda: mixedgemm.moe_plan(ids, E, expert_offsets=off, sorted_token=tok, slot_of=slot)),
                  gather=graph_time(lambda: mixedgemm.moe_gather(x, tok, out=xs)),
                  combine=graph_time(lambda: mixedgemm.moe_combine(y, ids, w, slot, out=out)))
        share = sum(us.values()) / block_us
        gb = 2 * T * K * H * 2 + 4 * T * K                    # every sorted row read and written, the token list
        cb = T * K * H * 2 + T * H * 2 + T * K * 10           # every expert row read, every token row written, ids / weights / slots
        counts = (off[1:] - off[:-1]).tolist()
        rows.append(dict(T=T, block_us=round(block_us, 1), loop_us=round(loop_us, 1), loop_ref_syncs_us=round(loop_sync_us, 1),
                         **{n + "_us": round(v, 2) for n, v in us.items()}, kernels_share=round(share, 4), gather_bytes=gb,
                         gather_tbps=round(gb / us["gather"] / 1e6, 3), combine_bytes=cb, combine_tbps=round(cb / us["combine"] / 1e6, 3),
                         rows_per_expert=counts))
        lines.append(f"{T:5d} {block_us:9.1f} {loop_us:9.1f} {loop_sync_us:20.1f} | {us['route']:7.2f} {us['plan']:7.2f} {us['gather']:7.2f} "
                     f"{us['combine']:8.2f} {share:6.3f} | {gb / us['gather'] / 1e6:9.2f} ({gb / us['gather'] / 8e6:5.3f}) "
                     f"{cb / us['combine'] / 1e6:10.2f} ({cb / us['combine'] / 8e6:5.3f})   {counts}")
    text = "\n".join(lines)
    print(text)
    print(json.dumps(rows))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; Mixtral-8x7B shapes H {H} I {I} E {E} top_k {K}\n{text}\n{json.dumps(rows)}\n")


def device_main(out_path):
    """SparseMoEBlock(capturable=True) against the default block (which is the parent's, line for line), one box, one run:
    per T the default block eager, the capturable block eager, both three times in alternation (the spread of each is printed), the
    capturable block as ONE graph replay, and the two new entries against the grouped calls they replace, each as ten calls in one
    graph (no host time): gather + grouped quantizer against moe_quantize, matmul_grouped against moe_matmul for w1 (N = I) and w2
    (N = H).  The possible costs of the device-sized form on their own: moe_matmul with max_rows = 64 on offsets whose groups all
    exceed 64 rows is the streaming launch in which every group exits; the tiled launch's grid bound against the tiles that exist."""
    dev = torch.device("cuda:0")
    experts = make_experts(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    gate_w = (torch.randn((E, H), generator=g, device=dev) * 0.05).to(torch.bfloat16)
    plain, capt = SparseMoEBlock(gate_w, experts, K), SparseMoEBlock(gate_w, experts, K, capturable=True)
    lines, rows = [], []
    for T in (1, 16, 128, 4096):
        x = torch.randn((T, H), generator=g, device=dev).to(torch.bfloat16)
        iters = 20 if T >= 4096 else 50
        same = torch.equal(plain(x)[0], capt(x)[0])      # (DESIGN.md 7e "Which bits": not on every routing once K > 512)
        eager = {"default": [], "capturable": []}
        for _ in range(3):
            eager["default"].append(timed(lambda: plain(x), iters))
            eager["capturable"].append(timed(lambda: capt(x), iters))
        replay = graph_time(lambda: capt(x), calls=1, iters=iters)
        ids, w = mixedgemm.moe_route(F.linear(x, gate_w), K)
        off, tok, slot = mixedgemm.moe_plan(ids, E)
        o = off.tolist()
        n = T * K
        cut = lambda t: [t[o[e]:o[e + 1]] for e in range(E)]
        t1, t3, t2 = capt._tables
        xs = mixedgemm.moe_gather(x, tok)
        q1 = mixedgemm.moe_quantize(x, tok, off, t1)
        q1g = mixedgemm.reorder_quantize_x_grouped(cut(xs), plain._idx1, *SPLIT_H)
        a, y = torch.empty((n, I), dtype=torch.bfloat16, device=dev), torch.empty((n, H), dtype=torch.bfloat16, device=dev)
        hbuf = torch.randn((n, I), generator=g, device=dev).to(torch.bfloat16)
        q2 = mixedgemm.moe_quantize(hbuf, None, off, t2)
        q2g = mixedgemm.reorder_quantize_x_grouped(cut(hbuf), plain._idx2, *SPLIT_I)
        us = {
            "gather + quantize_grouped (H)": graph_time(lambda: mixedgemm.reorder_quantize_x_grouped(cut(mixedgemm.moe_gather(x, tok, out=xs)), plain._idx1, *SPLIT_H)),
            "moe_quantize (H, gather inside)": graph_time(lambda: mixedgemm.moe_quantize(x, tok, off, t1, out=q1)),
            "quantize_grouped (I)": graph_time(lambda: mixedgemm.reorder_quantize_x_grouped(cut(hbuf), plain._idx2, *SPLIT_I)),
            "moe_quantize (I)": graph_time(lambda: mixedgemm.moe_quantize(hbuf, None, off, t2, out=q2)),
            "matmul_grouped w1": graph_time(lambda: mixedgemm.matmul_grouped(q1g, plain._B[0], outs=cut(a))),
            "moe_matmul w1": graph_time(lambda: mixedgemm.moe_matmul(q1, off, t1, T, out=a)),
            "matmul_grouped w2": graph_time(lambda: mixedgemm.matmul_grouped(q2g, plain._B[2], outs=cut(y))),
            "moe_matmul w2": graph_time(lambda: mixedgemm.moe_matmul(q2, off, t2, T, out=y)),
        }
        if min(c for c in (o[e + 1] - o[e] for e in range(E))) > 64:
            us["moe_matmul w1, max_rows 64: the streaming launch, every group exits"] = graph_time(lambda: mixedgemm.moe_matmul(q1, off, t1, 64, out=a))
        counts = [o[e + 1] - o[e] for e in range(E)]
        sp = lambda v: f"{min(v):8.1f} .. {max(v):8.1f}"
        lines.append(f"T = {T}: rows per expert {counts}; the two blocks' outputs are {'bit-equal' if same else 'NOT bit-equal'}")
        lines.append(f"  default block, eager      {sp(eager['default'])} us (three runs in alternation)")
        lines.append(f"  capturable block, eager   {sp(eager['capturable'])} us")
        lines.append(f"  capturable block, one graph replay {replay:8.1f} us")
        lines += [f"  {k:<72} {v:9.2f} us" for k, v in us.items()]
        rows.append(dict(T=T, rows_per_expert=counts, default_eager_us=[round(v, 1) for v in eager["default"]],
                         capturable_eager_us=[round(v, 1) for v in eager["capturable"]], capturable_replay_us=round(replay, 1),
                         entries_us={k: round(v, 2) for k, v in us.items()}))
    text = "\n".join(lines)
    print(text)
    print(json.dumps(rows))
    if out_path:
        with open(out_path, "w") as f:
            f.write(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; Mixtral-8x7B shapes H {H} I {I} E {E} top_k {K}\n{text}\n{json.dumps(rows)}\n")


def activate_main(out_path):
    """mixedgemm.moe_activate_quantize against the three launches it replaces (F.silu, *, moe_quantize), and
    SparseMoEBlock(capturable=True, fused_activation=True) against the capturable block (the parent's, line for line), one box, one
    run.  Per T: the three launches and the one, ten calls per hipGraph (no host time), three runs each in alternation (their spread is
    printed); the fused op's rate on its own 2 n I 2 input bytes as TB/s and as a fraction of 8 TB/s -- at T = 4 096 ten replays of
    0.47 GB exceed the 256 MiB Infinity Cache, so that one is an HBM rate; both blocks eager, three runs each in alternation, and each as
    ONE graph replay; and how many elements of h differ between the two (the device exp2 / rcp against torch's)."""
    dev = torch.device("cuda:0")
    experts = make_experts(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    gate_w = (torch.randn((E, H), generator=g, device=dev) * 0.05).to(torch.bfloat16)
    capt = SparseMoEBlock(gate_w, experts, K, capturable=True)
    fused = SparseMoEBlock(gate_w, experts, K, capturable=True, fused_activation=True)
    lines, rows = [], []
    for T in (1, 16, 128, 4096):
        x = torch.randn((T, H), generator=g, device=dev).to(torch.bfloat16)
        iters = 20 if T >= 4096 else 50
        n = T * K
        ids, w = mixedgemm.moe_route(F.linear(x, gate_w), K)
        off, tok, slot = mixedgemm.moe_plan(ids, E)
        t1, t3, t2 = capt._tables
        q1 = mixedgemm.moe_quantize(x, tok, off, t1)
        a, b = mixedgemm.moe_matmul(q1, off, t1, T), mixedgemm.moe_matmul(q1, off, t3, T)      # the op's real inputs
        h = torch.empty_like(a)
        q2 = mixedgemm.moe_activate_quantize(a, b, off, t2, h_out=h)
        differ = int((h.view(torch.int16) != (F.silu(a) * b).view(torch.int16)).sum())
        q3 = tuple(torch.empty_like(t) for t in q2)
        three = lambda: mixedgemm.moe_quantize(F.silu(a) * b, None, off, t2, out=q3)
        one = lambda: mixedgemm.moe_activate_quantize(a, b, off, t2, out=q2)
        op = {"three launches": [], "one launch": []}
        eager = {"capturable": [], "fused": []}
        for _ in range(3):
            op["three launches"].append(graph_time(three))
            op["one launch"].append(graph_time(one))
        for _ in range(3):
            eager["capturable"].append(timed(lambda: capt(x), iters))
            eager["fused"].append(timed(lambda: fused(x), iters))
        replay = {"capturable": graph_time(lambda: capt(x), calls=1, iters=iters), "fused": graph_time(lambda: fused(x), calls=1, iters=iters)}
        in_bytes = 2 * n * I * 2
        best = min(op["one launch"])
        sp = lambda v: f"{min(v):8.1f} .. {max(v):8.1f}"
        lines.append(f"T = {T} (n = {n}): {differ} of {n * I} elements of h differ from torch's F.silu(a) * b")
        lines.append(f"  F.silu, *, moe_quantize (ten per graph)     {sp(op['three launches'])} us (three runs in alternation)")
        lines.append(f"  moe_activate_quantize (ten per graph)       {sp(op['one launch'])} us: {in_bytes / best / 1e6:6.2f} TB/s on its {in_bytes / 1e6:.1f} MB of "
                     f"input, {in_bytes / best / 8e6:5.3f} of 8 TB/s")
        lines.append(f"  capturable block, eager                     {sp(eager['capturable'])} us")
        lines.append(f"  capturable block, fused activation, eager   {sp(eager['fused'])} us")
        lines.append(f"  one graph replay: capturable {replay['capturable']:8.1f} us, fused {replay['fused']:8.1f} us")
        rows.append(dict(T=T, h_elements_differing=differ, three_launches_us=[round(v, 2) for v in op["three launches"]],
                         one_launch_us=[round(v, 2) for v in op["one launch"]], input_bytes=in_bytes, input_tbps=round(in_bytes / best / 1e6, 3),
                         capturable_eager_us=[round(v, 1) for v in eager["capturable"]], fused_eager_us=[round(v, 1) for v in eager["fused"]],
                         replay_us={k: round(v, 1) for k, v in replay.items()}))
    text = "\n".join(lines)
    print(text)
    print(json.dumps(rows))
    if out_path:
        with open(out_path, "w") as f:
            f.write(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; Mixtral-8x7B shapes H {H} I {I} E {E} top_k {K}\n{text}\n{json.dumps(rows)}\n")


def gate_up_main(out_path):
    """mixedgemm.moe_gate_up_activate against the three launches it replaces -- two moe_matmul and moe_activate_quantize, the parent's
    code, never the code under test -- and SparseMoEBlock(capturable=True, fused_gate_up=True) against fused_activation=True, at
    T = 128, 1 024 and 4 096 on one box in one run.  Ten calls per hipGraph (no host time), three runs each in alternation so that the
    spread is seen; both blocks as ONE graph replay, three runs in alternation.  The bar at T = 4 096: the one launch is faster than the
    three by more than the spread between the runs."""
    dev = torch.device("cuda:0")
    experts = make_experts(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    gate_w = (torch.randn((E, H), generator=g, device=dev) * 0.05).to(torch.bfloat16)
    old = SparseMoEBlock(gate_w, experts, K, capturable=True, fused_activation=True)
    new = SparseMoEBlock(gate_w, experts, K, capturable=True, fused_gate_up=True)
    lines, rows = [], []
    for T in (128, 1024, 4096):
        x = torch.randn((T, H), generator=g, device=dev).to(torch.bfloat16)
        iters = 20 if T >= 1024 else 50
        n = T * K
        ids, w = mixedgemm.moe_route(F.linear(x, gate_w), K)
        off, tok, slot = mixedgemm.moe_plan(ids, E)
        t1, t3, t2 = old._tables
        q1 = mixedgemm.moe_quantize(x, tok, off, t1)
        a, b = mixedgemm.moe_matmul(q1, off, t1, T), mixedgemm.moe_matmul(q1, off, t3, T)
        q2 = mixedgemm.moe_activate_quantize(a, b, off, t2)
        q3 = mixedgemm.moe_gate_up_activate(q1, off, new._gate_up_table, T, SPLIT_I)
        counts = (off[1:] - off[:-1]).tolist()
        same = all(torch.equal(u[:n], v[:n]) for u, v in zip(q2[:3], q3[:3]))

        def three():
            mixedgemm.moe_matmul(q1, off, t1, T, out=a)
            mixedgemm.moe_matmul(q1, off, t3, T, out=b)
            mixedgemm.moe_activate_quantize(a, b, off, t2, out=q2)
        one = lambda: mixedgemm.moe_gate_up_activate(q1, off, new._gate_up_table, T, SPLIT_I, out=q3)
        op = {"three": [], "one": []}
        replay = {"fused_activation": [], "fused_gate_up": []}
        for _ in range(3):
            op["three"].append(graph_time(three))
            op["one"].append(graph_time(one))
        for _ in range(3):
            replay["fused_activation"].append(graph_time(lambda: old(x), calls=1, iters=iters))
            replay["fused_gate_up"].append(graph_time(lambda: new(x), calls=1, iters=iters))
        sp = lambda v: f"{min(v):8.1f} .. {max(v):8.1f}"
        spread = max(max(v) - min(v) for v in op.values())
        lines.append(f"T = {T} (n = {n}, rows per expert {counts}): {mixedgemm.moe_gate_up_activate_describe(new._gate_up_table, n)}; packed bytes equal: {same}")
        lines.append(f"  two moe_matmul + moe_activate_quantize (ten per graph)   {sp(op['three'])} us (three runs in alternation)")
        lines.append(f"  moe_gate_up_activate (ten per graph)                     {sp(op['one'])} us; gain {min(op['three']) - max(op['one']):8.1f} us worst case against a spread of {spread:.1f} us")
        lines.append(f"  one graph replay of the block: fused_activation {sp(replay['fused_activation'])} us, fused_gate_up {sp(replay['fused_gate_up'])} us")
        rows.append(dict(T=T, rows_per_expert=counts, three_launches_us=[round(v, 2) for v in op["three"]], one_launch_us=[round(v, 2) for v in op["one"]],
                         packed_bytes_equal=same, replay_us={k: [round(u, 1) for u in v] for k, v in replay.items()}))
    text = "\n".join(lines)
    print(text)
    print(json.dumps(rows))
    if out_path:
        with open(out_path, "w") as f:
            f.write(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; Mixtral-8x7B shapes H {H} I {I} E {E} top_k {K}\n{text}\n{json.dumps(rows)}\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "device":
        device_main(sys.argv[2] if len(sys.argv) > 2 else None)
    elif len(sys.argv) > 1 and sys.argv[1] == "activate":
        activate_main(sys.argv[2] if len(sys.argv) > 2 else None)
    elif len(sys.argv) > 1 and sys.argv[1] == "gate_up":
        gate_up_main(sys.argv[2] if len(sys.argv) > 2 else None)
    else:
        main()
