"""Record which mm_* symbols the valid calls of tests/test_wrapper_errors_kv_moe_gpu.py reach, call by call, as
tests/golden/wrapper_entries_v1.json.  Re-record only when a wrapper is meant to reach other entries, from a tree whose wrappers are
known to be right (the package found first on PYTHONPATH is the one recorded):

    python tools/record_wrapper_entries.py > tests/golden/wrapper_entries_v1.json

Needs the GPU: the calls run."""
import importlib.util
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.append(ROOT)
spec = importlib.util.spec_from_file_location("wrapper_cases", os.path.join(ROOT, "tests", "test_wrapper_errors_kv_moe_gpu.py"))
cases = importlib.util.module_from_spec(spec)
spec.loader.exec_module(cases)
json.dump(cases.record_entries(cases.operands(torch.device("cuda:0"))), sys.stdout, indent=1)
print()
