"""Call time of fused attention with per-sequence valid lengths against the
unmasked call, at B=64, H=12, D=64 and S=128 (full-S kernel) / S=512 (flash
kernel):
  (a) unmasked            (b) masked, all lens = S
  (c) masked, lens = S/4  (d) masked, lens uniform-random in [1, S] (seeded)

Every figure is a CALL time from a host clock around synchronised work: per
variant, ROUNDS windows of ITERS back-to-back calls, each window closed by a
synchronise, the variants alternating round by round so that clock drift
hits all of them alike. Printed per variant: the median window and the
min..max over windows (the run-to-run spread inside this process).

    python tools/bench_attn_varlen.py                  # all four variants
    python tools/bench_attn_varlen.py --unmasked-only  # (a) only: also runs
                                   # on a build that predates the lens argument
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import torch

from arkflow_amd.ops import require_native

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--iters", type=int, default=40)  # 10 x 40 = 400 per variant
ap.add_argument("--unmasked-only", action="store_true")
args = ap.parse_args()
assert args.rounds * args.iters >= 300

nat = require_native()
B, H, D = 64, 12, 64
dev = torch.device("cuda")

for S in (128, 512):
    g = torch.Generator().manual_seed(9900 + S)
    qkv = torch.randn(B, S, 3, H, D, generator=g).to(dev, torch.bfloat16)
    scale = D ** -0.5
    variants = {"a_unmasked": None}
    if not args.unmasked_only:
        variants["b_lens_full"] = torch.full((B,), S, dtype=torch.int32,
                                             device=dev)
        variants["c_lens_quarter"] = torch.full((B,), S // 4,
                                                dtype=torch.int32, device=dev)
        variants["d_lens_random"] = torch.randint(
            1, S + 1, (B,), generator=g).to(dev, torch.int32)

    def call(lens):
        if lens is None:
            return nat.attention_qkv_bf16(qkv, scale)
        return nat.attention_qkv_bf16(qkv, scale, lens=lens)

    for lens in variants.values():  # warm-up: code load, allocator, clocks
        for _ in range(50):
            call(lens)
    torch.cuda.synchronize()
    windows = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, lens in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                call(lens)
            torch.cuda.synchronize()
            windows[name].append((time.perf_counter() - t0) / args.iters * 1e6)
    base = statistics.median(windows["a_unmasked"])
    for name, w in windows.items():
        med = statistics.median(w)
        print(json.dumps({
            "S": S, "variant": name, "call_us_median": round(med, 2),
            "call_us_min": round(min(w), 2), "call_us_max": round(max(w), 2),
            "vs_unmasked": round(med / base, 3),
            "mean_len": None if variants[name] is None
            else round(float(variants[name].float().mean()), 1),
            "iters": args.rounds * args.iters}), flush=True)
