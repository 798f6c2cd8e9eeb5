"""The weight-streaming kernels' host side (csrc/mx_stream_plan.h), checked without a device.

tools/stream_plan_host_check.cpp is compiled with the host compiler and run three ways: its invariants over twelve CU counts between 1 and 1024;
its listing against tests/golden/stream_dispatch_v1.json; and its plan of the streaming shapes the GPU suite launches.

How the fixture was made.  It was recorded from the commit BEFORE mx_stream_plan.h existed, never from the code under test: in a
scratch copy of that commit each leaf launcher of mx_gemm_stream.hip (launch_one, launch_grouped_one, launch_moe_one, launch_quant,
launch_gate_up_act_tiles) was patched to print its template parameters and computed sizes and to return before touching the device,
and a small driver called the exported mm::launch_... / ..._supported entry points with null operands over the cases of
`stream_plan_host_check --cases`, one child process per override value (the overrides were cached in statics).  Without a device the
library plans for 256 CUs, the MI355X's count.  Neither the patch nor the driver is in the tree.  Layout: "cases" (one per line, the
checker's case syntax), "results" (the distinct answers), "index" (the answer of each case).

The one intended difference from the recording: a predicate no longer says yes to a shape whose launch is then refused (`narrowed`).
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "stream_dispatch_v1.json")
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
pytestmark = pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")

PLAIN_ONLY = {(4, 1, 2, 4), (1, 1, 4, 8)}
# every kernel the file instantiates, per kind: (F, T16, D, NW) and the weight modes ("w4": fp4 weights, "w": matching precision)
TIERS_ABOVE_16 = {(2, 2, 2, 4): ("w4",), (1, 2, 3, 8): ("w4", "w"), (1, 2, 2, 8): ("w4",), (2, 2, 3, 4): ("w4", "w"), (2, 3, 2, 4): ("w4", "w"),
                  (1, 3, 2, 8): ("w4", "w"), (2, 4, 2, 4): ("w4", "w"), (1, 4, 2, 8): ("w4", "w")}
GROUPED_LIST = {(2, 1, 2, 8): ("w4", "w"), (1, 1, 3, 8): ("w4", "w"), **TIERS_ABOVE_16}
PLAIN_LIST = {(4, 1, 2, 4): ("w4", "w"), (1, 1, 4, 8): ("w4", "w"), **GROUPED_LIST}
QUANT_LIST = {(4, 1, d, 4): ("w4", "w") for d in (2, 3, 4)} | {(2, 1, d, 8): ("w4", "w") for d in (2, 3, 4)} | {(1, 1, d, 8): ("w4", "w") for d in (3, 4)}
LISTS = {"plain": PLAIN_LIST, "grouped": GROUPED_LIST, "moe": GROUPED_LIST, "act": {(4, 1, 2, 4): ("w4",), (4, 2, 2, 4): ("w4",)}, "qlinear": QUANT_LIST,
         "down": {(2, 1, 2, 8): ("w4", "w"), (1, 1, 3, 8): ("w4", "w")}, "actq": {(4, 1, 2, 4): ("w4",)}}
# a row of the lists that no ladder picks: with fp4 weights 17 .. 32 tokens on 32 features run two slots, (2, 2, 2, 4)
NEVER_PICKED = {((2, 2, 3, 4), "w4")}
# ... and rows the launcher picks and mm_matmul never asks it for: 32 < M <= 64 goes to the tiles once N / 32 reaches the CUs
# (plan_small_m_uses_tiles), so a default plain launch never runs the 32-feature configurations of three and four token tiles
UNREACHED = {"plain": NEVER_PICKED | {((2, 3, 2, 4), "w4"), ((2, 3, 2, 4), "w"), ((2, 4, 2, 4), "w4"), ((2, 4, 2, 4), "w")}, "grouped": NEVER_PICKED, "moe": NEVER_PICKED}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stream_plan") / "stream_plan_host_check")
    subprocess.run([CXX, "-std=c++20", "-O1", os.path.join(ROOT, "tools", "stream_plan_host_check.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        fx = json.load(f)
    cases = fx["cases"].split("\n")
    assert fx["version"] == 1 and fx["cus"] == 256 and len(cases) == len(fx["index"])
    return [parse(c, fx["results"][i]) for c, i in zip(cases, fx["index"])]


def parse(case, result):
    """a line of the listing as a dict: kind, M, N, K, w ("w4" / "w"), groups, rows, norm, override, sup, and the launch (None: refused)"""
    t = case.split()
    ov = t.pop() if "=" in t[-1] else ""
    kind, v = t[0], [int(x) for x in t[1:]]
    d = {"case": case, "result": result, "kind": kind, "M": v.pop(0), "override": ov, "groups": 1, "rows": 0, "norm": 0}
    if kind == "grouped":
        d["groups"] = v.pop(0)
    if kind == "moe":
        d["groups"], d["rows"] = v.pop(0), v.pop(0)
    d["N"], d["K"] = v.pop(0), (v.pop(0), v.pop(0), v.pop(0))
    d["w"] = "w4" if kind in ("act", "actq") or v.pop(0) else "w"
    if kind in ("qlinear", "actq"):
        d["norm"] = v.pop(0)
    assert not v, case
    r = dict(p.split("=") for p in result.split() if "=" in p)
    d["sup"] = r.pop("sup") == "1"
    d["launch"] = None
    if "invalid" not in result:
        d["launch"] = {"cfg": tuple(int(x) for x in r["cfg"].split(",")), "var": r["var"], "grid": r["grid"], "lds": int(r["lds"]), "raise": r["raise"] == "1",
                       "rows": int(r.get("rows", -1)), "early": int(r.get("early", -1))}
    return d


def tier(m):
    return (min(m, 64) + 15) // 16


def narrowed(lines):
    """the cases the recording answers yes and the plan-asking predicates no: those whose own launch the recording refuses; a grouped
    query (it stands for either weight mode) when the launch of the other mode is refused; a device-sized query (it knows neither N nor
    the experts, and every tier below its own must be supported) when a grouped or device-sized launch of the same K at its tier or
    below is refused"""
    refused = [d for d in lines if d["sup"] and d["launch"] is None]
    grouped = {(d["M"], d["groups"], d["N"], d["K"], d["override"]) for d in refused if d["kind"] == "grouped"}
    tiers = {(d["K"], d["override"], tier(d["M"])) for d in refused if d["kind"] in ("grouped", "moe")}
    out = set()
    for d in lines:
        if not d["sup"]:
            continue
        if d["launch"] is None or (d["kind"] == "grouped" and (d["M"], d["groups"], d["N"], d["K"], d["override"]) in grouped) or (
                d["kind"] == "moe" and any((d["K"], d["override"], t) in tiers for t in range(1, tier(d["M"]) + 1))):
            out.add(d["case"])
    return out


def _other_cu_count():
    """the CU count of a present device when it is not the fixture's 256, else None"""
    import torch
    if not torch.cuda.is_available():
        return None
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus if cus != 256 else None


def test_plan_invariants_for_other_cu_counts(checker):
    run = subprocess.run([checker], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-2000:]


def test_listing_replays_the_recording(checker, recorded):
    cus = _other_cu_count()
    if cus is not None:
        pytest.skip(f"the fixture holds the plan for 256 CUs; this device has {cus}")
    got = subprocess.run([checker, "--list"], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(got) == len(recorded)
    no_longer = narrowed(recorded)
    assert 0 < len(no_longer) < len(recorded) // 20 and all(sum(d["K"]) >= 43008 or d["override"] for d in recorded if d["case"] in no_longer)
    diff = []
    for line, d in zip(got, recorded):
        want = d["result"].replace("sup=1", "sup=0") if d["case"] in no_longer else d["result"]
        if line != f"{d['case']} : {want}":
            diff.append((line, f"{d['case']} : {want}"))
    assert not diff, (len(diff), diff[:5])


def test_fixture_reaches_every_rung(recorded):
    """a narrower sweep cannot pass: every kernel of every kind's list, every predicate both ways, both sides of every threshold"""
    assert os.path.getsize(FIXTURE) < 256 * 1024
    ok = [d for d in recorded if d["launch"]]
    dflt = [d for d in ok if not d["override"]]
    for kind, rows in LISTS.items():
        seen = {(d["launch"]["cfg"], d["w"]) for d in ok if d["kind"] == kind}
        want = {(cfg, w) for cfg, ws in rows.items() for w in ws} - (NEVER_PICKED if kind in UNREACHED else set())
        assert seen == want, (kind, sorted(want - seen), sorted(seen - want))
        assert {d["sup"] for d in recorded if d["kind"] == kind and not d["override"]} == {True, False}, kind
    assert {d["launch"]["var"] for d in ok if d["kind"] in ("qlinear", "actq")} == {"Q", "RMS", "ADD", "ACT", "ACT+RMS", "ACT+ADD"}
    # every override, and each one changes an answer of its default twin
    base = {d["case"]: d["result"] for d in recorded if not d["override"]}
    ovs = {d["override"] for d in recorded if d["override"]}
    assert ovs == {"MICROMIX_STREAM=0", "MICROMIX_STREAM_GROUPED=0", "MICROMIX_STREAM_GROUPED_MAX_M=32", "MICROMIX_DECODE_STREAM=0", "MICROMIX_DECODE_STREAM=2",
                   "MICROMIX_DECODE_EARLY=0", "MICROMIX_DECODE_F4=-1", "MICROMIX_DECODE_F4=2", "MICROMIX_DECODE_F4=3", "MICROMIX_DECODE_F4=4",
                   "MICROMIX_DECODE_DEPTH=3", "MICROMIX_DECODE_DEPTH=4", "MICROMIX_GATE_UP_ACT_STREAM=0"}
    for ov in ovs:
        assert any(base[d["case"][: -len(ov) - 1]] != d["result"] for d in recorded if d["override"] == ov), ov
    # the thresholds of the ladders, on the plain launch: M = 8 | 9 (the predicate), 16 | 17, 32 | 33, 48 | 49, 64 | 65
    plain = {(d["M"], d["N"], d["K"], d["w"]): d for d in recorded if d["kind"] == "plain" and not d["override"]}
    K32, K33 = (2048, 128, 1920), (0, 0, 4224)
    assert not plain[(8, 4096, K32, "w4")]["sup"] and plain[(9, 4096, K32, "w4")]["sup"] and plain[(8, 4097, K32, "w4")]["sup"]
    assert [plain[(m, 4096, K32, "w4")]["launch"]["cfg"][1] for m in (16, 17, 32, 33, 48, 49, 64)] == [1, 2, 2, 3, 3, 4, 4]
    assert plain[(64, 4096, K32, "w4")]["sup"] and not plain[(65, 4096, K32, "w4")]["sup"]
    # wide and not (N / 32 against 256), more than two rounds and not (against 512), slabs 32 | 33
    assert [plain[(16, n, K32, "w")]["launch"]["cfg"] for n in (8160, 8192, 16384, 16416)] == [(1, 1, 4, 8), (2, 1, 2, 8), (2, 1, 2, 8), (4, 1, 2, 4)]
    assert plain[(16, 4096, K33, "w")]["launch"]["cfg"] == (1, 1, 3, 8)
    for kind in ("grouped", "moe"):      # the same tiers and widths without the two plain-only rules
        cfgs = {d["launch"]["cfg"] for d in dflt if d["kind"] == kind}
        assert not (cfgs & PLAIN_ONLY) and {c[:2] for c in cfgs} == {(f, t) for f in (1, 2) for t in (1, 2, 3, 4)}, kind
    # two_tile_fits(3, .) true and false
    assert {plain[(17, 4097, k, "w4")]["launch"]["cfg"] for k in ((0, 0, 26624), (0, 0, 26752))} == {(1, 2, 3, 8), (1, 2, 2, 8)}
    # the quantizing launches: rows staged in batches, the early phase on and off, both sides of wide / two rounds / 32 slabs
    quant = [d for d in dflt if d["kind"] in ("qlinear", "actq")]
    assert any(d["launch"]["rows"] < d["M"] for d in quant) and any(d["launch"]["rows"] == d["M"] > 1 for d in quant)
    assert {d["launch"]["early"] for d in quant} == {0, 1} and {d["launch"]["early"] for d in dflt if d["kind"] == "down"} == {0, 1}
    assert {d["launch"]["cfg"] for d in dflt if d["kind"] == "qlinear"} == {(4, 1, 2, 4), (2, 1, 2, 8), (1, 1, 4, 8), (1, 1, 3, 8)}
    assert {d["launch"]["raise"] for d in dflt} == {True, False}


# ---- the streaming shapes the GPU suite launches ----
def _gpu_suite_cases():
    """the checker's cases for STREAM_CASES, WIDE_M x WIDE_N, the n == 264 edge cases and the GROUPED and MOE tables of
    tests/test_gemm_exact_gpu.py, as mm_matmul / mm_matmul_grouped / mm_moe_matmul form their launches"""
    import test_gemm_exact_gpu as g
    out = []
    for M, N, split in g.STREAM_CASES:
        out += [f"plain {M} {N} {split[0]} {split[1]} {split[2]} {w}" for w in (1, 0)]
    out += [f"plain {M} {g.WIDE_N} {' '.join(map(str, g.EDGE_SPLIT))} {w}" for M in g.WIDE_M if M <= 16 for w in (1, 0)]
    out += [f"plain {M} 264 {' '.join(map(str, g.EDGE_SPLIT))} 1" for M in g.EDGE_M if M <= 64]
    for N, split, ms in g.GROUPED:      # groups of 1 .. 64 rows share launches of up to eight, in order (mm_matmul_grouped)
        small = [m for m in ms if 0 < m <= 64]
        for i in range(0, len(small), 8):
            chunk = small[i:i + 8]
            out += [f"grouped {max(chunk)} {len(chunk)} {N} {split[0]} {split[1]} {split[2]} {w}" for w in (1, 0)]
    for N, split, ms in g.MOE_TABLES:
        out += [f"moe {max(ms)} {len(ms)} {sum(ms)} {N} {split[0]} {split[1]} {split[2]} {w}" for w in (1, 0)]
    return out


def test_gpu_cases_reach_every_default_configuration(checker):
    """every kernel of the plain, grouped and device-sized lists that a default dispatch can pick is launched by a case of the GPU suite"""
    cases = _gpu_suite_cases()
    lines = subprocess.run([checker, "--plan", *cases], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == len(cases)
    got = [parse(*line.split(" : ")) for line in lines]
    assert all(d["sup"] and d["launch"] for d in got), [d["case"] for d in got if not (d["sup"] and d["launch"])]
    for kind in ("plain", "grouped", "moe"):
        seen = {(d["launch"]["cfg"], d["w"]) for d in got if d["kind"] == kind}
        want = {(cfg, w) for cfg, ws in LISTS[kind].items() for w in ws} - UNREACHED[kind]
        assert seen == want, (kind, "not launched:", sorted(want - seen), "unexpected:", sorted(seen - want))
