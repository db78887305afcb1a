"""String order on one GPU: the device path (csrc/bytes_order.hip) against
the host fallback it replaced, on the same device-resident batch.

    python tools/bench_bytes_order.py [--rows 8192,262144,1048576] [--out F]

Times ops.bytes_rank alone and three queries — ORDER BY s, min(s) per group,
WHERE s < literal — over three string shapes: short unique strings (8-12
bytes), long low-cardinality ids (32 bytes, 100 distinct) and ~200-byte
strings behind a 150-byte common prefix. The host fallback is the code the
executor ran before the device path existed (copy the column to the host,
order Python bytes objects); it is kept here only, and swapped into the
executor for the `host` timings. Call time is a host clock around
device-synchronised work: warm-up, then the two paths alternating, median over
the repeats (fewer for a slow call). `rounds` is the number of 7-byte chunk
rounds the rank needs for the shape (computed on the host from the data).
Prints one JSON line per (shape, rows).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from arkflow_amd import ops  # noqa: E402
from arkflow_amd.batch import Column, MessageBatch  # noqa: E402
from arkflow_amd.sql import engine as sql_engine  # noqa: E402
from arkflow_amd.sql import eval as sql_eval  # noqa: E402
from arkflow_amd.sql.engine import SqlExecutor  # noqa: E402

QUERIES = {
    "order_by": "SELECT * FROM flow ORDER BY s",
    "min_group": "SELECT k, min(s) FROM flow GROUP BY k",
    "where_lt": "SELECT * FROM flow WHERE s < '{lit}'",
}


# ------------------------------------------------------------------- data
def _fixed_width(rng, n, width, alphabet):
    return alphabet[rng.integers(0, len(alphabet), (n, width))]


def make_strings(shape: str, n: int, rng) -> list:
    hexd = np.frombuffer(b"0123456789abcdef", dtype=np.uint8)
    if shape == "short_unique":
        # unique through an 8-byte id, 16 ids to each 7-byte chunk, then a
        # random tail of 0-4 bytes
        tail = _fixed_width(rng, n, 4, hexd)
        lens = rng.integers(0, 5, n)
        return [b"s-%06x" % i + tail[i, :lens[i]].tobytes()
                for i in rng.permutation(n)]
    if shape == "long_low_card":
        ids = [b"device-id-%022d" % (i * 7919) for i in range(100)]
        return [ids[j] for j in rng.integers(0, 100, n)]
    if shape == "prefix_150":
        prefix = b"/var/log/streams/" + b"x" * 133
        body = _fixed_width(rng, n, 60, hexd)
        lens = rng.integers(30, 61, n)
        return [prefix + body[i, :lens[i]].tobytes() for i in range(n)]
    raise ValueError(shape)


def rank_rounds(rows: list) -> int:
    """Rounds of 7-byte chunks until every row is alone or finished."""
    srt = sorted(rows)
    need = 1
    for a, b in zip(srt, srt[1:]):
        # the pair is still open after round c (from 0) when both rows hold
        # the same c + 1 full chunks
        c = need - 1
        while len(a) >= 7 * (c + 1) and a[:7 * (c + 1)] == b[:7 * (c + 1)]:
            c += 1
        need = c + 1
    return need


# ------------------------------------- the host fallback the device replaced
def host_order_key(col: Column) -> torch.Tensor:
    vals = col.to_pylist()
    idx = sorted(range(len(vals)),
                 key=lambda i: vals[i] if vals[i] is not None else b"")
    rank = torch.empty(len(vals), dtype=torch.int64)
    rank[torch.tensor(idx)] = torch.arange(len(vals))
    return rank.to(col.data.device)


def host_min_max(arg: Column, gid, g: int, name: str) -> Column:
    pv = arg.to_pylist()
    gl = gid.detach().to("cpu").tolist()
    best = [None] * g
    for v, gi in zip(pv, gl):
        if v is None:
            continue
        b = best[gi]
        if b is None or (v < b if name == "min" else v > b):
            best[gi] = v
    return Column.from_bytes([b if b is not None else b"" for b in best]
                             ).to(arg.data.device)


def host_order_cmp(op: str, lv, rv, env) -> torch.Tensor:
    ls = lv.to_pylist()
    r = rv.encode()
    fn = {"<": lambda a: a < r, "<=": lambda a: a <= r,
          ">": lambda a: a > r, ">=": lambda a: a >= r}[op]
    return torch.tensor([fn(a) for a in ls], dtype=torch.bool,
                        device=env.device)


class host_fallback:
    """Swap the host fallback into the executor for the calls inside."""
    def __enter__(self):
        self.saved = (sql_engine._string_order_key,
                      sql_engine._string_min_max, sql_eval._string_order_cmp)
        sql_engine._string_order_key = host_order_key
        sql_engine._string_min_max = host_min_max
        sql_eval._string_order_cmp = host_order_cmp

    def __exit__(self, *exc):
        (sql_engine._string_order_key, sql_engine._string_min_max,
         sql_eval._string_order_cmp) = self.saved


# ------------------------------------------------------------------ timing
def timed(fn) -> float:
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def compare(dev_fn, host_fn, budget_s: float) -> dict:
    """Median call time of both, alternating; repeats sized to the budget."""
    for _ in range(3):
        dev_fn()
    torch.cuda.synchronize()
    first = timed(host_fn)
    reps = int(max(3, min(31, budget_s * 1e3 / max(first, 1e-3))))
    td, th = [], [first]
    for _ in range(reps):
        td.append(timed(dev_fn))
        if len(th) < reps:
            th.append(timed(host_fn))
    d, h = statistics.median(td), statistics.median(th)
    return {"device_ms": round(d, 3), "host_ms": round(h, 3),
            "host_over_device": round(h / d, 1), "repeats": reps}


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--rows", default="8192,262144,1048576")
    p.add_argument("--shapes",
                   default="short_unique,long_low_card,prefix_150")
    p.add_argument("--budget", type=float, default=4.0,
                   help="seconds of host-path repeats per measurement")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("needs a GPU: a CPU timing says nothing about this path")
    ops.require_native()
    dev = torch.device("cuda:0")
    lines = []
    for shape in a.shapes.split(","):
        for n in (int(x) for x in a.rows.split(",")):
            rng = np.random.default_rng(n)
            rows = make_strings(shape, n, rng)
            col = Column.from_bytes(rows).to(dev)
            batch = MessageBatch({
                "k": Column("numeric", torch.from_numpy(
                    rng.integers(0, 64, n))).to(dev),
                "v": Column("numeric", torch.from_numpy(
                    rng.random(n).astype(np.float32))).to(dev),
                "s": col,
            })
            lit = sorted(rows)[n // 2].decode()
            result = {"shape": shape, "rows": n,
                      "bytes": int(col.data.numel()),
                      "rounds": rank_rounds(rows)}

            def host_rank():
                with host_fallback():
                    sql_engine._string_order_key(col)

            same = torch.equal(
                ops.sort_indices(ops.bytes_rank(col)),
                ops.sort_indices(host_order_key(col)))
            result["order_equal"] = bool(same)
            result["bytes_rank"] = compare(lambda: ops.bytes_rank(col),
                                           host_rank, a.budget)
            for name, sql in QUERIES.items():
                ex = SqlExecutor(sql.format(lit=lit))

                def on_device():
                    return ex.execute({"flow": batch})

                def on_host():
                    with host_fallback():
                        return ex.execute({"flow": batch})

                result[name] = compare(on_device, on_host, a.budget)
                result[name]["rows_out"] = on_device().num_rows
            line = json.dumps(result)
            print(line, flush=True)
            lines.append(line)
            if a.out:
                with open(a.out, "w") as f:
                    f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
