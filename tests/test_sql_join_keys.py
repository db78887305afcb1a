"""Join, GROUP BY and ORDER BY on keys at the edges of their domain, against
SQLite: fractional REAL join keys (a cast to integer would join 1.5 with
1.2), INTEGER keys at -2^63 and 2^63-1 (the first is the hash tables' free
slot marker), and signed zeros as a sort key.

KEY_CASES is also run on the GPU against the CPU executor by
tests/test_sql_gpu_differential.py; `f32` there casts every REAL column to
float32 on both sides, which is what sends it through the native kernels."""
import sqlite3

import pytest
import torch

from arkflow_amd.batch import Column, MessageBatch
from arkflow_amd.sql.engine import SqlExecutor
from test_sql_differential import _normalize, _rows_close

I64_MIN = -(1 << 63)
I64_MAX = (1 << 63) - 1

# table name -> (sqlite column types, columns)
REAL_TABLES = {
    "ta": ("x REAL, i INTEGER",
           {"x": [1.5, 2.25, -0.5, 3.0, 0.5, 2.25, 7.75],
            "i": [0, 1, 2, 3, 4, 5, 6]}),
    "tb": ("y REAL, j INTEGER",
           {"y": [1.2, 2.25, 0.5, 3.9, 2.25, -0.25, 7.75],
            "j": [0, 1, 2, 3, 5, 6, 4]}),
}
LIMIT_TABLES = {
    "t": ("k INTEGER, v REAL",
          {"k": [I64_MIN, 3, I64_MAX, I64_MIN, 0, -1, I64_MAX, I64_MIN,
                 I64_MIN + 1, I64_MAX - 1, 3],
           "v": [0.5, 1.0, -2.5, 4.0, 8.0, 0.25, 16.0, -32.0, 1.5, 2.5,
                 64.0]}),
    "u": ("k INTEGER, w INTEGER",
          {"k": [I64_MAX, I64_MIN, 7, I64_MIN, 0, I64_MAX - 1],
           "w": [10, 20, 30, 40, 50, 60]}),
}
ZERO_TABLES = {
    "z": ("x REAL, y INTEGER",
          {"x": [0.0, -0.0, 1.0, -0.0, 0.0, -1.0, -0.0, 0.0, 1.0, -0.0],
           "y": [5, 3, 9, 8, 1, 0, 2, 7, 4, 6]}),
}

KEY_CASES = [
    (REAL_TABLES, "SELECT a.i, b.j FROM ta a JOIN tb b ON a.x = b.y "
                  "ORDER BY a.i, b.j"),
    (REAL_TABLES, "SELECT a.i, b.j FROM ta a LEFT JOIN tb b ON a.x = b.y "
                  "ORDER BY a.i, b.j"),
    (REAL_TABLES, "SELECT a.i, b.j FROM ta a JOIN tb b ON a.x + 0.25 = b.y "
                  "ORDER BY a.i, b.j"),
    (REAL_TABLES, "SELECT a.i, b.y FROM ta a JOIN tb b ON a.x = b.y "
                  "AND a.i = b.j ORDER BY a.i"),
    (REAL_TABLES, "SELECT a.i, b.y FROM ta a JOIN tb b ON a.i = b.j "
                  "AND a.x = b.y ORDER BY a.i"),
    (LIMIT_TABLES, "SELECT k, count(*) AS c, sum(v) AS s, min(v) AS lo, "
                   "max(v) AS hi FROM t GROUP BY k ORDER BY k"),
    (LIMIT_TABLES, "SELECT k, count(*) AS c FROM t GROUP BY k "
                   "ORDER BY k DESC"),
    (LIMIT_TABLES, "SELECT a.k, a.v, b.w FROM t a JOIN u b ON a.k = b.k "
                   "ORDER BY a.k, a.v, b.w"),
    (LIMIT_TABLES, "SELECT a.k, b.w FROM t a LEFT JOIN u b ON a.k = b.k "
                   "ORDER BY a.k, a.v, b.w"),
    (LIMIT_TABLES, "SELECT a.v, b.w FROM t a JOIN u b ON a.k = b.k "
                   "AND a.k + 0 = b.k + 0 ORDER BY a.v, b.w"),
    (ZERO_TABLES, "SELECT x, y FROM z ORDER BY x, y"),
    (ZERO_TABLES, "SELECT x, y FROM z ORDER BY x DESC, y DESC"),
    (ZERO_TABLES, "SELECT y, row_number() OVER (PARTITION BY x ORDER BY y) "
                  "AS rn FROM z ORDER BY y"),
]


def batches(tables, f32=False, device=None):
    out = {}
    for name, (_, cols) in tables.items():
        b = MessageBatch.from_dict(cols)
        if f32:
            b = b.with_columns({
                k: Column("numeric", c.data.float(), validity=c.validity)
                for k, c in b.columns.items()
                if c.kind == "numeric" and c.data.dtype == torch.float64})
        out[name] = b if device is None else b.to(device)
    return out


def _sqlite(tables, sql):
    conn = sqlite3.connect(":memory:")
    for name, (schema, cols) in tables.items():
        conn.execute(f"CREATE TABLE {name} ({schema})")
        marks = ",".join("?" * len(cols))
        conn.executemany(f"INSERT INTO {name} VALUES ({marks})",
                         list(zip(*cols.values())))
    rows = conn.execute(sql).fetchall()
    conn.close()
    return rows


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("tables,sql", KEY_CASES,
                         ids=[c[1] for c in KEY_CASES])
def test_key_edges_vs_sqlite(tables, sql, f32):
    out = SqlExecutor(sql).execute(batches(tables, f32))
    ours = [tuple(r.values()) for r in out.to_rows()]
    theirs = _sqlite(tables, sql)
    # every value these queries return is exact in float32
    assert _rows_close(_normalize(ours), _normalize(theirs)), \
        f"{sql}\n{ours}\nvs\n{theirs}"
    assert _normalize(ours) == _normalize(theirs)


def test_real_join_matches_exactly_one_fractional_pair():
    """1.5 / 1.2 and -0.5 / 0.5 collide after truncation; only 2.25 joins."""
    flow = {"a": MessageBatch.from_dict({"x": [1.5, 2.25, 3.0, -0.5]}),
            "b": MessageBatch.from_dict({"y": [1.2, 2.25, 3.9, 0.5]})}
    out = SqlExecutor("SELECT a.x, b.y FROM a JOIN b ON a.x = b.y"
                      ).execute(flow)
    assert [tuple(r.values()) for r in out.to_rows()] == [(2.25, 2.25)]
