#!/usr/bin/env python3
"""Flagship serving benchmark: generate → sql(filter) → ML inference → drop.

Measures the BASELINE.json headline metric — rows/sec (+ p50 pipeline
latency) for the generate→sql→infer pipeline — on N GPUs of one node, one
rank per GPU over RCCL (weak scaling: each rank runs an independent stream
shard, matching the engine's stream-per-GPU sharding model).

  python bench.py --gpus N --steps K --warmup W [--model mlp|bert]
                  [--batch-size 8192] [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the result line.
--dump-outputs DIR also writes what the last timed step returned, one
DIR/<column>.npy per output column, so two builds can be compared output for
output (the generator and the weights are seeded: same arguments, same
inputs). --full is where everything beyond the headline figure belongs;
today the benchmark measures nothing else, so it adds nothing.

One step = one batch of --batch-size rows through the full pipeline
(synthetic generator data, random-init weights; bf16 inference compute).
Rank 0 prints ONE JSON line per the driver contract.
"""
import argparse
import asyncio
import json
import os
import statistics
import time

import numpy as np
import torch


def build_pipeline(args, device):
    import arkflow_amd  # noqa: F401  (registers components)
    from arkflow_amd.inputs.generate import GenerateInput
    from arkflow_amd.processors.sql import SqlProcessor
    from arkflow_amd.processors.inference import InferenceProcessor
    from arkflow_amd.pipeline import Pipeline

    n_features = args.features
    fields = {f"f{i}": {"dtype": "float32", "low": 0.0, "high": 1.0}
              for i in range(n_features)}
    fields["key"] = {"dtype": "int64", "low": 0, "high": 1024}
    gen = GenerateInput({
        "batch_size": args.batch_size,
        "interval": "0ms",
        "fields": fields,
        "device": str(device),
        "seed": 7 + args.rank,
    })
    # filter keeps ~80% of rows, then per-row MLP scoring (or BERT per-seq)
    sql = SqlProcessor({"query": "SELECT * FROM flow WHERE f0 >= 0.2"})
    if args.model == "bert":
        gen_tok = GenerateInput({
            "batch_size": args.batch_size,
            "interval": "0ms",
            "fields": {"token": {"dtype": "int64", "low": 0, "high": 30000},
                       "f0": {"dtype": "float32", "low": 0.0, "high": 1.0}},
            "device": str(device),
            "seed": 7 + args.rank,
        })
        infer = InferenceProcessor({
            "model": "bert_base", "seq_len": 128, "device": str(device),
        })
        # BERT consumes whole batches (no filter — sequences must stay full)
        return gen_tok, Pipeline([infer])
    if args.model == "sqlagg":
        # BASELINE config 2: sql filter + hash aggregate, GPU-resident columns
        if device.type == "cuda" and not args.no_stepgraph:
            # whole-step hipGraph: generate+filter+group-by+reduce replay as
            # ONE graph, one CPU read (the host-mapped group count) per step
            from arkflow_amd.ops.stepgraph import (
                FusedGenerateAgg, FusedStepSource)

            def make_agg(seed_off=0):
                return FusedGenerateAgg(
                    fields, args.batch_size, "f0", ">=", 0.2, "key",
                    [("key", None, "key"), ("count", None, "c"),
                     ("sum", "f0", "s")], device,
                    seed=7 + args.rank + seed_off * 1000)

            seeds = iter(range(1, 16))
            src = FusedStepSource(
                make_agg(0),
                ninstances=int(os.environ.get("ARKFLOW_NINST", "2")),
                make_instance=lambda: make_agg(next(seeds)))
            return src, Pipeline([])
        agg = SqlProcessor({
            "query": "SELECT key, count(*) AS c, sum(f0) AS s FROM flow "
                     "WHERE f0 >= 0.2 GROUP BY key"})
        return gen, Pipeline([agg])
    if args.model == "proto_mlp":
        # BASELINE config 3: kafka-shaped protobuf payloads → GPU varint
        # decode → MLP anomaly scoring
        from arkflow_amd.batch import MessageBatch
        from arkflow_amd.processors.proto_wire import (
            ProtoSchema, encode_message)
        from arkflow_amd.processors.protobuf_proc import (
            ProtobufToArrowProcessor)
        import random
        proto = ("message T { double f0 = 1; double f1 = 2; double f2 = 3; "
                 "double f3 = 4; int64 key = 5; }")
        schema = ProtoSchema.parse(proto)
        rng = random.Random(42 + args.rank)
        payloads = [
            encode_message({"f0": rng.random(), "f1": rng.random(),
                            "f2": rng.random(), "f3": rng.random(),
                            "key": rng.randrange(1024)}, schema)
            for _ in range(args.batch_size)
        ]
        device_batch = MessageBatch.from_binary(
            payloads, input_name="kafka").to(device)

        class _ProtoGen:
            """Kafka-shaped source: device-resident wire-format payloads."""

            async def read(self):
                from arkflow_amd.spi import NoopAck
                return device_batch, NoopAck()

        if device.type == "cuda" and not args.no_stepgraph:
            # decode+featpack+MLP replay as one hipGraph (zero host syncs
            # per step — row count is fixed; same kernels as the eager path,
            # numerics-tested in tests/test_gpu_kernels.py)
            from arkflow_amd.models.mlp import MlpAnomalyDetector
            from arkflow_amd.ops.stepgraph import FusedProtoMlp
            from arkflow_amd.processors.protobuf_proc import build_gpu_spec
            fno, kind, isf, slot, int_f, float_f, str_f = \
                build_gpu_spec(schema)
            assert not str_f
            col = device_batch.column("__value__")
            mlp = MlpAnomalyDetector(len(float_f),
                                     [args.hidden, args.hidden], device,
                                     1234)
            fused = FusedProtoMlp(col.data, col.offsets, fno, kind, isf,
                                  slot, len(int_f), len(float_f), float_f,
                                  int_f, mlp, device)

            class _FusedProtoSrc:
                async def read(self):
                    from arkflow_amd.spi import NoopAck
                    return fused.step(), NoopAck()

            return _FusedProtoSrc(), Pipeline([])
        decode = ProtobufToArrowProcessor({"proto": proto}, None)
        infer = InferenceProcessor({
            "model": "mlp_anomaly", "columns": ["f0", "f1", "f2", "f3"],
            "hidden": [args.hidden, args.hidden], "device": str(device),
        })
        return _ProtoGen(), Pipeline([decode, infer])
    if device.type == "cuda" and not args.no_stepgraph:
        # whole-step hipGraph: generate+filter+MLP replay as ONE graph —
        # kills the host-dispatch ceiling at small batches.
        # Same work, same outputs as the eager path (numerics-tested in
        # tests/test_gpu_kernels.py).
        from arkflow_amd.models.mlp import MlpAnomalyDetector
        from arkflow_amd.ops.stepgraph import (
            FusedGenerateFilterInfer, FusedStepSource)
        mlp = MlpAnomalyDetector(n_features, [args.hidden, args.hidden],
                                 device, 1234)

        def make(seed_off=0):
            return FusedGenerateFilterInfer(
                fields, args.batch_size, "f0", ">=", 0.2, mlp, device,
                seed=7 + args.rank + seed_off * 1000)

        # two graph instances software-pipeline inside the source; the
        # engine loop itself stays sequential (workers=1)
        seeds = iter(range(1, 16))
        src = FusedStepSource(
            make(0), ninstances=int(os.environ.get("ARKFLOW_NINST", "2")),
            make_instance=lambda: make(next(seeds)))
        return src, Pipeline([])
    infer = InferenceProcessor({
        "model": "mlp_anomaly",
        "columns": [f"f{i}" for i in range(n_features)],
        "hidden": [args.hidden, args.hidden],
        "device": str(device),
    })
    return gen, Pipeline([sql, infer])


async def run_steps(gen, pipeline, n_steps, workers=1):
    """Process n_steps batches. workers>1 pipelines steps concurrently the
    way the engine's thread_num processor workers do (stream.py), overlapping
    host dispatch of step k+1 with device execution of step k; per-step
    latency (p50) is still measured per batch with a sync. Also returns the
    batches the LAST step produced (views into the step's static buffers —
    valid until the next read)."""
    rows = 0
    times = []
    last = []

    loop = asyncio.get_running_loop()

    async def one_step():
        nonlocal rows, last
        t0 = time.perf_counter()
        batch, ack = await gen.read()
        outs = last = await pipeline.process(batch)
        for b in outs:
            rows += b.num_rows
        if batch.device.type == "cuda":
            ev = torch.cuda.Event()
            ev.record()
            if workers <= 1:
                # serial loop: the fused source already synced its stream,
                # so the event is (near-)complete — skip the thread hop
                ev.synchronize()
            else:
                # event-based wait in an executor thread so OTHER in-flight
                # steps keep dispatching while this one drains (a blocking
                # torch.cuda.synchronize would stall the whole event loop)
                await loop.run_in_executor(None, ev.synchronize)
        times.append(time.perf_counter() - t0)
        await ack.ack()

    if workers <= 1:
        for _ in range(n_steps):
            await one_step()
        return rows, times, last

    sem = asyncio.Semaphore(workers)

    async def guarded():
        async with sem:
            await one_step()

    await asyncio.gather(*[guarded() for _ in range(n_steps)])
    return rows, times, last


DUMP_BUDGET_BYTES = 64 << 20  # ceiling for everything --dump-outputs writes


def dump_outputs(outs, out_dir):
    """Write the columns of the last step's output batches as
    out_dir/<column>.npy — float32, or float64 where float32 would lose
    bits (int64 / float64 columns). Binary columns are written as their
    byte and offset arrays. An array over its share of the 64 MB budget is
    cut to a fixed, seeded sample of its elements (sorted indices, so order
    is kept)."""
    arrays = {}
    for i, b in enumerate(outs):
        pre = "" if len(outs) == 1 else f"out{i}_"
        for name, col in b.columns.items():
            if col.kind == "binary":
                arrays[f"{pre}{name}.bytes"] = col.data
                arrays[f"{pre}{name}.offsets"] = col.offsets
            else:
                arrays[pre + name] = col.data
    os.makedirs(out_dir, exist_ok=True)
    if not arrays:
        return
    share = DUMP_BUDGET_BYTES // len(arrays)
    for name, t in arrays.items():
        wide = t.dtype in (torch.int64, torch.float64)
        t = t.detach().reshape(-1)
        cap = share // (8 if wide else 4) - 32  # leave room for the header
        if t.numel() > cap:
            idx = np.sort(np.random.default_rng(0).choice(
                t.numel(), size=cap, replace=False))
            t = t[torch.from_numpy(idx).to(t.device)]
        a = t.to(torch.float64 if wide else torch.float32).cpu().numpy()
        np.save(os.path.join(out_dir, name + ".npy"), a)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--batch-size", type=int, default=8192)
    p.add_argument("--model", choices=["mlp", "bert", "sqlagg", "proto_mlp"],
                   default="mlp")
    p.add_argument("--features", type=int, default=16)
    p.add_argument("--hidden", type=int, default=256)
    p.add_argument("--workers", type=int, default=1,
                   help="concurrent in-flight steps (engine thread_num analog)")
    p.add_argument("--no-stepgraph", action="store_true",
                   help="disable the whole-step hipGraph for --model mlp")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write the last step's "
                        "output columns as DIR/<column>.npy")
    p.add_argument("--full", action="store_true",
                   help="also run whatever the benchmark measures beyond "
                        "the headline figure (nothing today)")
    args = p.parse_args()

    args.rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local_rank = int(os.environ.get("LOCAL_RANK", args.rank))
    dist = None
    if world > 1:
        import torch.distributed as dist_mod
        dist = dist_mod
        backend = "nccl" if torch.cuda.is_available() else "gloo"
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        dist.init_process_group(backend=backend)
    if torch.cuda.is_available():
        device = torch.device("cuda", local_rank)
        torch.cuda.set_device(device)
    else:
        device = torch.device("cpu")

    gen, pipeline = build_pipeline(args, device)
    loop = asyncio.new_event_loop()

    # warmup (untimed)
    loop.run_until_complete(run_steps(gen, pipeline, args.warmup,
                                      args.workers))

    # timed region: barrier + sync on both sides
    if dist:
        dist.barrier()
    if device.type == "cuda":
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    rows, times, last = loop.run_until_complete(
        run_steps(gen, pipeline, args.steps, args.workers))
    if device.type == "cuda":
        torch.cuda.synchronize()
    if dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0

    if args.dump_outputs and args.rank == 0:
        dump_outputs(last, args.dump_outputs)

    # aggregate across ranks: MAX elapsed, SUM rows
    if dist:
        t = torch.tensor([elapsed], dtype=torch.float64,
                         device=device if device.type == "cuda" else "cpu")
        r = torch.tensor([float(rows)], dtype=torch.float64, device=t.device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dist.all_reduce(r, op=dist.ReduceOp.SUM)
        elapsed = float(t.item())
        rows = int(r.item())

    # rows/sec counts INPUT rows processed per wall-second across the job
    input_rows = args.steps * args.batch_size * world
    value = input_rows / elapsed
    p50_ms = statistics.median(times) * 1000.0
    p99_ms = (sorted(times)[max(0, int(len(times) * 0.99) - 1)] * 1000.0
              if times else 0.0)

    if args.rank == 0:
        print(json.dumps({
            "metric": "rows/sec",
            "value": value,
            "unit": "rows/s",
            "n_gpus": world if world > 1 else args.gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1000.0,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            # compute dtype: MFMA bf16 for the inference models; the
            # sql-aggregate path reduces in f32 (>= the reference's CPU f32)
            "dtype": "fp32" if args.model == "sqlagg" else "bf16",
            "data": "synthetic",
            "p50_ms": p50_ms,
            "p99_ms": p99_ms,
            "config": {
                "model": {
                    "mlp": "generate→sql(filter)→mlp_anomaly[16→256→256→1]",
                    "bert": "generate→bert_base(12L,768H,seq128)",
                    "sqlagg": "generate→sql(filter+hash_agg by 1024 keys)",
                    "proto_mlp": "kafka-shaped→protobuf_decode→mlp_anomaly",
                }[args.model],
                "global_batch": args.batch_size * max(world, args.gpus),
                "seq_len": 128 if args.model == "bert" else 1,
                "parallelism": f"dp{world if world > 1 else args.gpus}",
                "batch_size_per_gpu": args.batch_size,
                "workers": args.workers,
                "p50_ms": p50_ms,
                "filter": "WHERE f0 >= 0.2" if args.model == "mlp" else None,
            },
        }))
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
