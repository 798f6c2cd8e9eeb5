"""The tiled GEMM's host side, checked without a device.

Dispatch replay: tests/golden/gemm_dispatch_v1.json holds what mm_matmul_describe / mm_matmul_workspace_bytes, mm_gate_up_activate_describe /
_workspace_bytes and mm_moe_gate_up_activate_describe answered over a sweep of shapes, flags and developer overrides
(tools/record_gemm_dispatch.py, recorded before csrc/mx_gemm_plan.h gathered the rules); the current library must answer the same, byte
for byte.  The fixture is for 256 CUs -- what the library plans for without a device, and the MI355X's count.

Plan invariants for other CU counts: tools/gemm_plan_host_check.cpp, compiled with the host compiler and run here.
"""
import importlib.util
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "gemm_dispatch_v1.json")


def _recorder():
    spec = importlib.util.spec_from_file_location("record_gemm_dispatch", os.path.join(ROOT, "tools", "record_gemm_dispatch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _other_cu_count():
    """the CU count of a present device when it is not the fixture's 256, else None"""
    import torch
    if not torch.cuda.is_available():
        return None
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus if cus != 256 else None


@pytest.fixture(scope="module")
def recorded():
    rec = _recorder()
    with open(FIXTURE) as f:
        return rec, rec.unpack(json.load(f))


def test_fixture_reaches_every_kind(recorded):
    """a narrower sweep cannot pass: the whole issue's sweep is there, and every tile kind, both weight-streaming kernels, the tail
    split with and without the ping-pong loop and both split-K forms occur in it"""
    rec, want = recorded
    assert os.path.getsize(FIXTURE) < 256 * 1024
    base = want["base"]["matmul"]
    assert len(base) == len(list(rec.rows())) == 8 * 5 * 2 * 6 and all(len(r) == len(rec.MS) == 26 for r in base)
    assert len(want["base"]["gate_up"]) == 18 and len(want["base"]["moe"]) == 36
    assert sorted(want["overrides"]) == sorted(f"{n}={v}" for n, v in rec.OVERRIDES) and len(rec.OVERRIDES) == 16
    assert all(len(rows) == len(base) and all(len(r) == 7 for r in rows) for rows in want["overrides"].values())
    strings = {s for r in base for s, _ in r}
    marks = {
        "TK_SPLITK": ") + mm::splitk_reduce_kernel", "TK_SMALL_SPLIT": "(64x64 tiles, in-kernel split-K", "TK_G64": "(128x128 tiles)",
        "TK_G256_TAIL": "tile columns as 128x256 tiles)", "TK_G256": "(256x256 tiles)", "TK_G128": "(128x256 tiles)", "TK_G32": "(64x128 tiles)",
        "TK_G32N": "(64x64 tiles)", "TK_G16": "(32x64 tiles)", "stream": "mm::stream::mx_gemm_stream_kernel", "skinny": "mm::skinny::mx_gemm_skinny",
        "tail + ping-pong": "tile columns as 128x256 tiles), ping-pong K loop",
    }
    for what, mark in marks.items():
        assert any(mark in s for s in strings), what
    assert any(s.endswith("tile columns as 128x256 tiles)") for s in strings)              # the tail split without the ping-pong mark
    assert any(s.endswith("(256x256 tiles)") for s in strings) and any(s.endswith("(256x256 tiles), ping-pong K loop") for s in strings)
    pinned = {s for r in want["overrides"]["MICROMIX_SPLIT_SMALL=32:4"] for s, _ in r}
    assert any("(64x128 tiles, in-kernel split-K 4)" in s for s in pinned)                 # the only way to the 64 x 128 in-kernel split
    assert any(b > 0 for r in base for _, b in r)


def test_dispatch_replay(recorded):
    cus = _other_cu_count()
    if cus is not None:
        pytest.skip(f"the fixture holds the plan for 256 CUs; this device has {cus}")
    rec, want = recorded
    got = rec.sweep_all()
    assert got["base"]["gate_up"] == want["base"]["gate_up"]
    assert got["base"]["moe"] == want["base"]["moe"]
    keys = [(n, k, w, f, ws) for n, k, w, (f, ws) in rec.rows()]
    for name, ms, g, w in [("base", rec.MS, got["base"]["matmul"], want["base"]["matmul"])] + [
            (o, rec.MS[::4], got["overrides"][o], want["overrides"][o]) for o in sorted(want["overrides"])]:
        diff = [(name, m, *key, a, b) for key, gr, wr in zip(keys, g, w) for m, a, b in zip(ms, gr, wr) if a != b]
        assert not diff, (len(diff), diff[:5])


@pytest.mark.skipif(shutil.which("c++") is None and shutil.which("g++") is None and shutil.which("clang++") is None, reason="needs a host C++ compiler")
def test_plan_invariants_for_other_cu_counts(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    exe = str(tmp_path / "gemm_plan_host_check")
    subprocess.run([cxx, "-std=c++20", "-O1", os.path.join(ROOT, "tools", "gemm_plan_host_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-2000:]
