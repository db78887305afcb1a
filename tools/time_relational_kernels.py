"""Time radix_argsort (f32, 1M keys) and segment_reduce_f32 min (1M rows; 64
and 50 000 groups) of ONE build of the extension, given by the path of its
_native shared object, and print one JSON line. To compare two builds, run it
once per build in alternation, several times each; the `_check` fields must
agree between builds.

    python tools/time_relational_kernels.py <path/to/_native*.so> <label>
"""
import importlib.util
import json
import statistics
import sys

import torch

path, label = sys.argv[1], sys.argv[2]
spec = importlib.util.spec_from_file_location("_native", path)
nat = importlib.util.module_from_spec(spec)
spec.loader.exec_module(nat)
dev = torch.device("cuda:0")
torch.manual_seed(0)
n = 1 << 20
keys = torch.randn(n, device=dev)
vals = torch.randn(n, device=dev)
g64 = torch.randint(0, 64, (n,), device=dev, dtype=torch.int32)
g50k = torch.randint(0, 50_000, (n,), device=dev, dtype=torch.int32)
work = {
    "sort_f32_1M": lambda: nat.radix_argsort(keys, False),
    "segmin_1M_g64": lambda: nat.segment_reduce_f32(vals, g64, 64, 1),
    "segmin_1M_g50k": lambda: nat.segment_reduce_f32(vals, g50k, 50_000, 1),
}
out = {"label": label}
for name, fn in work.items():
    for _ in range(20):
        r = fn()
    torch.cuda.synchronize()
    windows = []
    iters = 300
    for _ in range(7):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            r = fn()
        b.record()
        torch.cuda.synchronize()
        windows.append(a.elapsed_time(b) * 1000.0 / iters)
    out[name + "_us"] = round(statistics.median(windows), 2)
    out[name + "_min_us"] = round(min(windows), 2)
    out[name + "_check"] = float(r.double().sum().item())
print(json.dumps(out), flush=True)
