"""The activation quantizers' host side (csrc/mx_quant_plan.h), checked without a device.

tools/quant_plan_host_check.cpp is compiled with the host compiler and run two ways: its invariants -- what the kernels of
reorder_quantize.hip, rmsnorm_quantize.hip and qlinear_decode.hip rely on and state only in comments -- over twelve CU counts between 1
and 1024 and every K that is a multiple of 128 up to 32768; and its listing against tests/golden/quant_dispatch_v1.json.

How the fixture was made.  It was recorded from the commit BEFORE mx_quant_plan.h existed, never from the code under test: in a scratch
copy of that commit DynamicLdsOnce::ensure, OccupancyCache::get, MM_LAUNCH and hipLaunchKernelGGL (all reached through mx_kernels.h)
were replaced by functions that print the kernel handed to them (its demangled name, found from the pointer with dladdr), the threads,
the LDS bytes, the kernel and byte count handed to `ensure` (or none), the grid, and what the kernel is told (the ring's slot bytes,
the decode launch's staged rows), and that return before touching the device.  A small driver called the seven launchers of the three
files with null operands over the cases of `quant_plan_host_check --cases`, one child process per override value (the overrides are
cached in statics) and per answer of the occupancy query, 1 and 6; the decode launcher was recorded with the streaming kernel's
predicate answering no, so that every case reaches its own launch.  Without a device the library plans for 256 CUs, the MI355X's count.
Neither the patch nor the driver is in the tree.  Layout: "cases_sha256" (of the output of `--cases`, which the answers follow in order; the list itself is the checker's), "kernels" (the names),
"results" (the distinct answers: kernel, threads, LDS bytes, raised kernel:bytes or -, grid, grid for an occupancy of 6, then slot= /
rows=; `expand` gives the checker's line), "index" (the answer of each case).

The one intended difference from the recording: the dynamic-LDS limit is raised on the kernel that is launched (`raised_on_launched`).
The recording raises it on the matching-precision 1024-thread kernel of the family whatever it launches.
"""
import hashlib
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "quant_dispatch_v1.json")
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
pytestmark = pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")

LIST_K = (128, 384, 4096, 8192, 8320, 16384, 16512, 20480, 24576, 24704, 28672, 32768)
LIST_ROWS = (0, 1, 2, 512, 513, 4096)
REORDER_FAMILY = ("reorder", "grouped", "moe", "moeact")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("quant_plan") / "quant_plan_host_check")
    subprocess.run([CXX, "-std=c++20", "-O1", os.path.join(ROOT, "tools", "quant_plan_host_check.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def recorded(checker):
    with open(FIXTURE) as f:
        fx = json.load(f)
    text = subprocess.run([checker, "--cases"], capture_output=True, text=True, check=True).stdout.rstrip("\n")
    cases = text.split("\n")
    # the cases the answers were recorded for, in that order
    assert fx["version"] == 1 and fx["cus"] == 256 and len(cases) == len(fx["index"]) and hashlib.sha256(text.encode()).hexdigest() == fx["cases_sha256"]
    return [parse(c, expand(fx["results"][i], fx["kernels"])) for c, i in zip(cases, fx["index"])]


def expand(result, kernels):
    """a stored answer as the checker prints it"""
    if result in ("none", "error"):
        return result
    k, thr, lds, r, grid, grid6, *extra = result.split()
    raised = "none" if r == "-" else kernels[int(r.split(":")[0])] + ":" + r.split(":")[1]
    return " ".join([f"kern={kernels[int(k)]} thr={thr} lds={lds} raise={raised} grid={grid} grid6={grid6}", *extra])


def parse(case, result):
    """a line of the listing as a dict: kind, mode, rows (grouped: the largest group's; moe: slots; decode: M), groups, N, K, split, int,
    add, norm, w4, override, and the launch (None: no launch; "error": refused)"""
    t = case.split()
    ov = t.pop() if "=" in t[-1] else ""
    kind = t.pop(0)
    d = {"case": case, "result": result, "kind": kind, "override": ov, "mode": t.pop(0) if kind in ("reorder", "grouped", "moe") else "", "groups": 1, "N": 0,
         "int": 1, "add": 0, "norm": 0}
    v = [int(x) for x in t]
    d["rows"] = v.pop(0)
    if kind == "grouped":
        d["groups"] = v.pop(0)
    if kind == "decode":
        d["N"] = v.pop(0)
    else:
        d["K"] = v.pop(0)
    d["split"] = (v.pop(0), v.pop(0), v.pop(0))
    if kind == "decode":
        d["K"], d["norm"], w4 = sum(d["split"]), v.pop(0), v.pop(0)
        d["mode"] = "w4" if w4 else "w"
    if kind == "rms":
        d["int"], d["add"] = v.pop(0), v.pop(0)
    assert not v, case
    d["launch"] = None if result == "none" else result
    if result not in ("none", "error"):
        r = dict(p.split("=") for p in result.split())
        d["launch"] = {"kern": r["kern"], "thr": int(r["thr"]), "lds": int(r["lds"]), "raise": r["raise"], "grid": r["grid"], "grid6": r["grid6"],
                       "slot": int(r.get("slot", 0)), "rows": int(r.get("rows", 0))}
    return d


def raised_on_launched(lines):
    """the cases whose limit the recording raises on another kernel than the one it launches: fp4 weights on the 1024-thread kernels of
    reorder_quantize.hip once the staged row passes 48 KiB, K > 24576"""
    return {d["case"] for d in lines if d["kind"] in REORDER_FAMILY and d["mode"] == "w4" and d["K"] > 24576 and isinstance(d["launch"], dict)}


def test_plan_invariants(checker):
    run = subprocess.run([checker], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-2000:]
    assert re.fullmatch(r"\d{6,} cases checked; 0 failures\n", run.stdout), run.stdout[-400:]


def test_listing_replays_the_recording(checker, recorded):
    got = subprocess.run([checker, "--list"], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(got) == len(recorded)
    moved = raised_on_launched(recorded)
    # exactly the cases the recording itself shows raising on another kernel than it launches
    assert moved == {d["case"] for d in recorded if isinstance(d["launch"], dict) and d["launch"]["raise"] != "none"
                     and d["launch"]["raise"].split(":")[0] != d["launch"]["kern"]}
    assert moved and all(d["launch"]["thr"] > 256 and d["launch"]["kern"].endswith("<true,1024>") for d in recorded if d["case"] in moved)
    diff = []
    for line, d in zip(got, recorded):
        want = d["result"]
        if d["case"] in moved:
            want = want.replace("raise=" + d["launch"]["raise"], "raise=" + d["launch"]["kern"] + ":" + d["launch"]["raise"].split(":")[1])
        if line != f"{d['case']} : {want}":
            diff.append((line, f"{d['case']} : {want}"))
    assert not diff, (len(diff), diff[:5])


def test_fixture_reaches_every_rung(recorded):
    """a narrower sweep cannot pass: every kernel the three files instantiate, both sides of every threshold, every override"""
    assert os.path.getsize(FIXTURE) < 128 * 1024
    ok = [d for d in recorded if isinstance(d["launch"], dict)]
    seen = {d["launch"]["kern"] for d in ok}
    tf = ("true", "false")
    want = {f"{fam}<{w},{t}>" for fam in ("reorder_quantize_kernel", "reorder_quantize_grouped_kernel", "moe_quantize_kernel") for w in tf for t in (256, 1024)}
    want |= {f"moe_activate_quantize_kernel<{t}>" for t in (256, 1024)}
    want |= {f"rmsnorm_quantize_ring_kernel<{i},{r}>" for i in tf for r in (3, 4)}      # (no ring with the residual)
    want |= {f"rmsnorm_quantize_products_kernel<{i},{s}>" for i in tf for s in ("RowLoad", "RowAddResidual")}
    want |= {f"rmsnorm_quantize_kernel<{i},{g},{s}>" for i in tf for g in (1, 2) for s in ("RowLoad", "RowAddResidual")}
    variants = (("false", "false"), ("true", "false"), ("true", "true"))      # plain, norm, residual add + norm
    want |= {f"qlinear_decode{f}_kernel<{w},{rms},{lpg},{add}>" for f in ("", "16") for w in tf for rms, add in variants for lpg in (1, 2)}
    assert seen == want, (sorted(want - seen), sorted(seen - want))
    # the cases the issue sets
    for kind in ("reorder", "rms"):
        assert {(d["K"], d["rows"]) for d in recorded if d["kind"] == kind} >= {(k, r) for k in LIST_K for r in LIST_ROWS}, kind
    assert {d["mode"] for d in recorded if d["kind"] == "reorder"} == {"x", "w", "w4"}
    assert {(d["int"], d["add"]) for d in recorded if d["kind"] == "rms"} == {(i, a) for i in (0, 1) for a in (0, 1)}
    assert {d["override"] for d in recorded} == {"", "MICROMIX_RMS_RING=0", "MICROMIX_RMS_RING=3", "MICROMIX_RMS_RING=4", "MICROMIX_DECODE_PERSIST=0"}
    assert {d["groups"] for d in recorded if d["kind"] == "grouped"} == {1, 3, 8}
    dec = [d for d in recorded if d["kind"] == "decode"]
    assert {d["rows"] for d in dec} == set(range(1, 9)) and {d["N"] for d in dec} == {4096, 8192, 14336, 28672} and len({d["split"] for d in dec}) == 3
    assert {(d["norm"], d["mode"]) for d in dec} == {(n, w) for n in (0, 1, 2) for w in ("w", "w4")}
    # rows = 0 launches nothing; a grouped launch without rows is refused
    assert all((d["launch"] is None) == (d["rows"] == 0) for d in recorded if d["kind"] in ("reorder", "rms", "moe", "moeact"))
    assert all((d["launch"] == "error") == (d["rows"] == 0) for d in recorded if d["kind"] == "grouped")
    # the ring's boundary, 512 = 2 x 256 rows, and its pins; never with the residual, never beyond K = 8192
    rms = {(d["rows"], d["K"], d["add"], d["override"]): d["launch"]["kern"] for d in ok if d["kind"] == "rms" and d["int"] and d["split"][0] not in (0, d["K"])}
    assert "ring_kernel<true,3>" in rms[(512, 4096, 0, "")] and "products" in rms[(513, 4096, 0, "")] and "products" in rms[(512, 4096, 1, "")]
    assert "products" in rms[(1, 4096, 0, "MICROMIX_RMS_RING=0")] and "ring_kernel<true,4>" in rms[(513, 4096, 0, "MICROMIX_RMS_RING=4")]
    assert "products" in rms[(1, 4096, 1, "MICROMIX_RMS_RING=3")]
    assert "ring_kernel<true,3>" in rms[(1, 8192, 0, "")] and "rmsnorm_quantize_kernel<true,1," in rms[(1, 8320, 0, "MICROMIX_RMS_RING=3")]
    assert "kernel<true,1," in rms[(1, 16384, 0, "")] and "kernel<true,2," in rms[(1, 16512, 0, "")]
    assert all(d["launch"]["slot"] > 0 for d in ok if "ring" in d["launch"]["kern"]) and not any("ring" in d["launch"]["kern"] for d in ok if d["add"] or d["K"] > 8192)
    # the limit is raised and not; the occupancy answer changes a grid and not; the decode launch stages all rows and fewer, persists and not
    assert {d["launch"]["raise"] == "none" for d in ok if d["kind"] != "decode"} == {True, False}
    assert {d["launch"]["grid"] == d["launch"]["grid6"] for d in ok if d["kind"] in ("reorder", "grouped", "rms")} == {True, False}
    assert any(d["launch"]["rows"] < d["rows"] for d in dec) and any(d["launch"]["rows"] == d["rows"] > 1 for d in dec)
    base = {d["case"]: d["result"] for d in dec if not d["override"]}
    assert any(base[d["case"].rsplit(" ", 1)[0]] != d["result"] for d in dec if d["override"])
