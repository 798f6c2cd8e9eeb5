"""reorder_quantize with fp4 weights and more than 48 KiB of LDS as the FIRST launch of a process.

The launcher raises the dynamic-LDS limit on the kernel it launches (launch_kernel, csrc/mx_kernels.h).  Every other test of these
shapes runs in a process where some kernel of the family has had its limit raised before; here a fresh child process launches
reorder_quantize_kernel<true, 1024> before anything else -- K = 32768, the top of the range, then K = 24704, the first K above the
48 KiB threshold -- and both outputs are compared with the oracle byte for byte, as tests/test_quantize_gpu.py compares them.
Three rows: the smallest count with more than one row per workgroup stride.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
CASES = [(3, 32768, (16384, 8192, 8192)), (3, 24704, (24704, 0, 0))]      # in launch order


def inputs(rows, k):
    from conftest import make_inputs
    rng = np.random.default_rng(rows * 131 + k)
    return make_inputs(rng, rows, k, "weight"), rng.permutation(k).astype(np.int16)


def child(out_path):
    """uploads are copies and the outputs come from torch.empty: the two quantizer launches are the process's first two kernels"""
    import torch
    from micromix_amd import mixedgemm
    dev = torch.device("cuda:0")
    got = []
    for rows, k, split in CASES:
        xb, idx = inputs(rows, k)
        x = torch.from_numpy(np.ascontiguousarray(xb).view(np.int16).copy()).view(torch.bfloat16).to(dev)
        got.append(mixedgemm.reorder_quantize_w4(x, torch.from_numpy(idx).to(dev), *split))
    torch.cuda.synchronize()
    np.savez(out_path, **{f"case{n}_{i}": t.cpu().numpy() for n, out in enumerate(got) for i, t in enumerate(out)})
    print("done", flush=True)


def test_first_launch_raises_the_limit_on_the_launched_kernel(dev, tmp_path):
    from oracle import mx_oracle as o
    from test_quantize_gpu import assert_quant_equal
    out = str(tmp_path / "first_launch.npz")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), out], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "done" in p.stdout, (p.stdout[-1500:], p.stderr[-1500:])
    got = np.load(out)
    for n, (rows, k, split) in enumerate(CASES):
        xb, idx = inputs(rows, k)
        assert_quant_equal([got[f"case{n}_{i}"] for i in range(6)], o.reorder_quantize(xb, idx, *split, "w4"), rows, split, f"w4 {rows}x{k} {split}")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    child(sys.argv[1])
