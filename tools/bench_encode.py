"""Throughput microbench for the GPU protobuf encoder: `arrow_to_protobuf`
on a device-resident batch, device path (`encoder: auto`) against the per-row
host codec on the same batch (`encoder: host`: device-to-host copy of every
column + one encode_message call per row). Run on a GPU box:
    python tools/bench_encode.py [--json]
"""
import argparse
import asyncio
import json
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

from arkflow_amd.batch import Column, MessageBatch
from arkflow_amd.processors.protobuf_proc import ArrowToProtobufProcessor

# the five-field schema bench.py builds for --model proto_mlp
NUMERIC = ("message T { double f0 = 1; double f1 = 2; double f2 = 3; "
           "double f3 = 4; int64 key = 5; }")
WITH_STRING = NUMERIC.replace(" }", " string body = 6; }")
MIN_WINDOW_S = 1.0  # each timed window runs at least this long

dev = torch.device("cuda:0")
loop = asyncio.new_event_loop()


def make_batch(n, with_string):
    g = torch.Generator().manual_seed(42)
    cols = {f"f{i}": Column("numeric",
                            torch.rand(n, generator=g, dtype=torch.float64))
            for i in range(4)}
    cols["key"] = Column("numeric", torch.randint(0, 1024, (n,), generator=g))
    if with_string:
        # ~200 bytes, lengths 184..215 so payload starts take every alignment
        cols["body"] = Column.from_bytes(
            [((b"lorem ipsum dolor sit amet %07d " % i) * 7)[:184 + i % 32]
             for i in range(n)])
    return MessageBatch(cols).to(dev)


def window(proc, batch, iters):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        out, = loop.run_until_complete(proc.process(batch))
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e-3 / iters, out


def measure(proc, batch, warmup):
    for _ in range(warmup):
        loop.run_until_complete(proc.process(batch))
    per_call, _ = window(proc, batch, 1)
    if per_call < 10e-3:  # one short call is mostly its own start-up
        per_call, _ = window(proc, batch, 100)
    iters = max(3, math.ceil(MIN_WINDOW_S / per_call))
    per_call, out = window(proc, batch, iters)
    return per_call, iters, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", action="store_true",
                    help="also print one JSON line with every figure")
    ap.add_argument("--rows", type=int, nargs="*", default=[8192, 262144])
    args = ap.parse_args()
    results = []
    print(f"{'schema':22s} {'rows':>7s}  {'device rows/s':>14s} {'GB/s':>7s} "
          f"{'ms':>8s}   {'host rows/s':>12s} {'ms':>9s}  {'speedup':>8s}")
    for label, proto, with_string in (
            ("5 numeric", NUMERIC, False),
            ("5 numeric + 200B str", WITH_STRING, True)):
        for n in args.rows:
            batch = make_batch(n, with_string)
            t_dev, it_dev, out = measure(
                ArrowToProtobufProcessor({"proto": proto}), batch, warmup=5)
            t_host, it_host, ref = measure(
                ArrowToProtobufProcessor({"proto": proto, "encoder": "host"}),
                batch, warmup=1)
            value = out.columns["__value__"]
            assert value.data.is_cuda, "device path not taken"
            assert value.to_pylist() == ref.binary_values()
            nbytes = int(value.data.numel())
            r = {"schema": label, "rows": n, "out_bytes": nbytes,
                 "device_ms": t_dev * 1e3, "device_iters": it_dev,
                 "device_rows_per_s": n / t_dev,
                 "device_out_gb_per_s": nbytes / t_dev / 1e9,
                 "host_ms": t_host * 1e3, "host_iters": it_host,
                 "host_rows_per_s": n / t_host,
                 "speedup": t_host / t_dev}
            results.append(r)
            print(f"{label:22s} {n:7d}  {r['device_rows_per_s'] / 1e6:12.1f} M "
                  f"{r['device_out_gb_per_s']:7.2f} {r['device_ms']:8.3f}   "
                  f"{r['host_rows_per_s'] / 1e6:10.3f} M {r['host_ms']:9.1f}  "
                  f"{r['speedup']:7.0f}x", flush=True)
    if args.json:
        print(json.dumps({"bench": "proto_encode", "results": results}))


if __name__ == "__main__":
    main()
