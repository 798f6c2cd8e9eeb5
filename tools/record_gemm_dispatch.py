"""Record what the tiled GEMM's host side decides -- the describe strings and workspace sizes of mm_matmul, mm_gate_up_activate and
mm_moe_gate_up_activate -- over a sweep of shapes, flags and developer overrides, for tests/test_gemm_dispatch_cpu.py.

    python tools/record_gemm_dispatch.py [tests/golden/gemm_dispatch_v1.json]

Needs no GPU: without a device the library plans for 256 CUs, the MI355X's count (a device with another count gives other answers).
The overrides are read once per process, so each one is swept in a child process of its own.

Fixture layout (strings and rows stored once): "strings"; "pairs" = [string index, workspace bytes]; "rows" = the pair indices of one
(N, K, wmode, flags) over the M list; every sweep is a list of row indices in the order of rows() below.
"""
import itertools
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

MS = (1, 16, 17, 32, 33, 64, 65, 96, 128, 129, 192, 256, 257, 384, 512, 513, 768, 1024, 1025, 1536, 2048, 2049, 3072, 4000, 4096, 8192)
NS = (256, 1024, 2048, 3000, 4096, 6144, 14336, 28672)
KS = ((0, 0, 4096), (2048, 128, 1920), (0, 0, 128), (1024, 1024, 12288), (0, 0, 256))
ROUND_ONCE, SPLIT_K_ALWAYS, TICKETS_ZEROED, OUT_F32 = 1, 2, 4, 8
FLAGS_WS = ((0, 0), (0, 1 << 30), (TICKETS_ZEROED, 1 << 30), (SPLIT_K_ALWAYS, 1 << 30), (SPLIT_K_ALWAYS | TICKETS_ZEROED, 1 << 30),
            (OUT_F32 | ROUND_ONCE, 0))
ACT_MS, ACT_IS = (16, 64, 65, 128, 2048, 4096), (1024, 7168, 14336)
MOE_ES, MOE_NS, MOE_IS = (1, 8, 64), (1, 771, 3400, 20000), (384, 1024, 7168)
OVERRIDES = [("MICROMIX_GEMM_TILE", v) for v in ("16", "32", "33", "64", "128", "256")] + [
    ("MICROMIX_GEMM_TAIL", "0"), ("MICROMIX_GEMM_TILE16", "0"), ("MICROMIX_SPLITK", "0"), ("MICROMIX_SPLITK", "4"),
    ("MICROMIX_SPLIT_SMALL", "0"), ("MICROMIX_SPLIT_SMALL", "33:4"), ("MICROMIX_SPLIT_SMALL", "32:4"),
    ("MICROMIX_SMALL_M_TILES", "1"), ("MICROMIX_MID_M_STREAM", "1"), ("MICROMIX_SMALL_M_TILE16", "0")]
OVERRIDE_NAMES = sorted({n for n, _ in OVERRIDES})


def rows():
    """every (N, K, wmode, flags, workspace bytes) of the sweep; the M list runs inside each"""
    return itertools.product(NS, KS, (0, 1), FLAGS_WS)


def sweep_matmul(lib, ms):
    """[[(describe string, workspace bytes) for M in ms] for row in rows()]"""
    out = []
    for n, (kn, ks, ko), wmode, (flags, ws) in rows():
        out.append([(lib.mm_matmul_describe(m, n, kn, ks, ko, wmode, flags, ws).decode(),
                     lib.mm_matmul_workspace_bytes(m, n, kn, ks, ko, wmode, flags)) for m in ms])
    return out


def sweep_act(lib):
    return [(lib.mm_gate_up_activate_describe(m, i).decode(), lib.mm_gate_up_activate_workspace_bytes(m, i))
            for m in ACT_MS for i in ACT_IS]


def sweep_moe(lib):
    return [lib.mm_moe_gate_up_activate_describe(e, n, i).decode() for e in MOE_ES for n in MOE_NS for i in MOE_IS]


def sweep_process(reduced):
    """what this process's library answers (the overrides in its environment included), as plain lists"""
    from micromix_amd import _lib
    lib = _lib.load()
    if reduced:
        return {"matmul": sweep_matmul(lib, MS[::4])}
    return {"matmul": sweep_matmul(lib, MS), "gate_up": sweep_act(lib), "moe": sweep_moe(lib)}


def sweep_child(name, value):
    """the reduced sweep (every fourth M) in a child process with one override set and every other one unset"""
    env = {k: v for k, v in os.environ.items() if k not in OVERRIDE_NAMES}
    env[name] = value
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, check=True, capture_output=True, text=True).stdout
    return [[tuple(p) for p in row] for row in json.loads(out)["matmul"]]


def sweep_all():
    """{"base": {...}, "overrides": {"NAME=value": matmul rows}} of the current library"""
    stale = [n for n in OVERRIDE_NAMES if n in os.environ]
    if stale:
        raise RuntimeError(f"unset {stale} first: the base sweep is the library's own choice")
    return {"base": sweep_process(False), "overrides": {f"{n}={v}": sweep_child(n, v) for n, v in OVERRIDES}}


class Table:
    def __init__(self, items=()):
        self.items = [tuple(x) if isinstance(x, list) else x for x in items]
        self.index = {x: i for i, x in enumerate(self.items)}

    def add(self, x):
        if x not in self.index:
            self.index[x] = len(self.items)
            self.items.append(x)
        return self.index[x]


def pack(result):
    strings, pairs, rws = Table(), Table(), Table()
    pair = lambda p: pairs.add((strings.add(p[0]), p[1]))
    row = lambda r: rws.add(tuple(pair(p) for p in r))
    base = result["base"]
    return {"version": 1, "cus": 256,
            "base": {"matmul": [row(r) for r in base["matmul"]], "gate_up": [pair(p) for p in base["gate_up"]],
                     "moe": [strings.add(s) for s in base["moe"]]},
            "overrides": {k: [row(r) for r in v] for k, v in result["overrides"].items()},
            "strings": strings.items, "pairs": pairs.items, "rows": rws.items}


def unpack(fixture):
    strings, pairs, rws = fixture["strings"], fixture["pairs"], fixture["rows"]
    pair = lambda i: (strings[pairs[i][0]], pairs[i][1])
    row = lambda i: [pair(j) for j in rws[i]]
    base = fixture["base"]
    return {"base": {"matmul": [row(i) for i in base["matmul"]], "gate_up": [pair(i) for i in base["gate_up"]],
                     "moe": [strings[i] for i in base["moe"]]},
            "overrides": {k: [row(i) for i in v] for k, v in fixture["overrides"].items()}}


if __name__ == "__main__":
    if "--child" in sys.argv:
        json.dump(sweep_process(True), sys.stdout)
        sys.exit(0)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "gemm_dispatch_v1.json"))
    result = sweep_all()
    fixture = pack(result)
    assert unpack(fixture) == result
    with open(path, "w") as f:
        json.dump(fixture, f, separators=(",", ":"))
        f.write("\n")
    cases = sum(len(r) for r in result["base"]["matmul"])
    print(f"{path}: {cases} mm_matmul cases, {len(fixture['strings'])} distinct strings, {os.path.getsize(path)} bytes")
