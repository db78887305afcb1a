"""Window frames (ROWS BETWEEN ...) on the CPU executor: differential against
SQLite, fp64 brute force for random frames, parser errors, and the contextual
frame words."""
import random
import sqlite3
import zlib

import pytest
import torch

from arkflow_amd import ops
from arkflow_amd.batch import MessageBatch
from arkflow_amd.sql.engine import SqlExecutor
from arkflow_amd.sql.parser import SqlError, parse_sql
from test_sql_differential import _normalize, _rows_close

FRAMES = [
    "ROWS BETWEEN 2 PRECEDING AND CURRENT ROW",
    "ROWS BETWEEN 1 PRECEDING AND 1 FOLLOWING",
    "ROWS BETWEEN 3 PRECEDING AND 1 PRECEDING",   # empty on first rows
    "ROWS BETWEEN 1 FOLLOWING AND 4 FOLLOWING",   # empty on last rows
    "ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW",
    "ROWS BETWEEN CURRENT ROW AND UNBOUNDED FOLLOWING",
    "ROWS BETWEEN UNBOUNDED PRECEDING AND UNBOUNDED FOLLOWING",
    "ROWS 5 PRECEDING",
    "ROWS BETWEEN 500 PRECEDING AND 500 FOLLOWING",  # wider than a partition
    "ROWS BETWEEN 2 FOLLOWING AND UNBOUNDED FOLLOWING",
    "ROWS BETWEEN UNBOUNDED PRECEDING AND 2 PRECEDING",
]
FUNCS = ["sum(a)", "count(*)", "count(a)", "avg(b)", "min(b)", "max(a)",
         "first_value(a)", "last_value(b)"]


def _all_funcs(over):
    cols = ", ".join(f"{f} OVER ({over}) AS f{i}"
                     for i, f in enumerate(FUNCS))
    return f"SELECT id, {cols} FROM flow ORDER BY id"


QUERIES = [_all_funcs(f"PARTITION BY k ORDER BY id {fr}") for fr in FRAMES] + [
    # DESC, a two-key order (unique through id), no PARTITION BY
    _all_funcs("PARTITION BY k ORDER BY id DESC "
               "ROWS BETWEEN 2 PRECEDING AND 1 FOLLOWING"),
    _all_funcs("PARTITION BY k ORDER BY c DESC, id "
               "ROWS BETWEEN 1 PRECEDING AND 2 FOLLOWING"),
    _all_funcs("ORDER BY id ROWS BETWEEN 6 PRECEDING AND CURRENT ROW"),
    # two frames of one function in one SELECT must not share a result
    "SELECT id, sum(c) OVER (PARTITION BY k ORDER BY id ROWS BETWEEN 1 "
    "PRECEDING AND CURRENT ROW) AS s1, sum(c) OVER (PARTITION BY k ORDER BY "
    "id ROWS BETWEEN 3 PRECEDING AND CURRENT ROW) AS s3, sum(c) OVER "
    "(PARTITION BY k ORDER BY id) AS s FROM flow ORDER BY id",
    # unaliased: the output names carry the frame too
    "SELECT id, max(c) OVER (ORDER BY id ROWS 1 PRECEDING), max(c) OVER "
    "(ORDER BY id ROWS 2 PRECEDING) FROM flow ORDER BY id",
    # a frame inside an expression
    "SELECT id, c - avg(c) OVER (PARTITION BY k ORDER BY id ROWS BETWEEN 2 "
    "PRECEDING AND 2 FOLLOWING) AS d FROM flow ORDER BY id",
    # the two RANGE forms, on the running and the whole-partition path
    "SELECT id, sum(c) OVER (PARTITION BY k ORDER BY id RANGE BETWEEN "
    "UNBOUNDED PRECEDING AND CURRENT ROW) AS r, max(c) OVER (PARTITION BY k "
    "ORDER BY id RANGE UNBOUNDED PRECEDING) AS m FROM flow ORDER BY id",
    "SELECT id, sum(c) OVER (PARTITION BY k ORDER BY id RANGE BETWEEN "
    "UNBOUNDED PRECEDING AND UNBOUNDED FOLLOWING) AS r, count(*) OVER "
    "(PARTITION BY k ORDER BY id RANGE BETWEEN UNBOUNDED PRECEDING AND "
    "UNBOUNDED FOLLOWING) AS n, last_value(c) OVER (PARTITION BY k ORDER BY "
    "id RANGE BETWEEN UNBOUNDED PRECEDING AND UNBOUNDED FOLLOWING) AS lv "
    "FROM flow ORDER BY id",
    # the rank family and lag accept a frame and ignore it
    "SELECT id, row_number() OVER (PARTITION BY k ORDER BY id ROWS BETWEEN 1 "
    "PRECEDING AND CURRENT ROW) AS rn, lag(c, 1, -1) OVER (PARTITION BY k "
    "ORDER BY id ROWS 2 PRECEDING) AS lg FROM flow ORDER BY id",
]


def _table(rng, n, nulls):
    """8 partitions; id is a shuffled row id, so ORDER BY id is unique within
    every partition and ROWS results do not depend on tie order."""
    def maybe(v):
        return None if nulls and rng.random() < 0.25 else v
    ids = list(range(n))
    rng.shuffle(ids)
    return {
        "id": ids,
        "a": [maybe(rng.randrange(100)) for _ in range(n)],
        "b": [maybe(round(rng.random(), 6)) for _ in range(n)],
        "c": [rng.randrange(-5, 6) for _ in range(n)],
        "k": [rng.randrange(8) for _ in range(n)],
    }


def _sqlite(data, sql):
    conn = sqlite3.connect(":memory:")
    conn.execute("CREATE TABLE flow (id INTEGER, a INTEGER, b REAL, "
                 "c INTEGER, k INTEGER)")
    conn.executemany("INSERT INTO flow VALUES (?,?,?,?,?)",
                     list(zip(*(data[c] for c in "id a b c k".split()))))
    rows = conn.execute(sql).fetchall()
    conn.close()
    return rows


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("n", [1, 17, 200])
@pytest.mark.parametrize("qi", range(len(QUERIES)))
def test_frames_vs_sqlite(qi, n, nulls):
    sql = QUERIES[qi]
    rng = random.Random(qi * 100 + n + nulls)
    data = _table(rng, n, nulls)
    out = SqlExecutor(sql).execute({"flow": MessageBatch.from_dict(data)})
    ours = _normalize([tuple(r.values()) for r in out.to_rows()])
    theirs = _normalize(_sqlite(data, sql))
    assert _rows_close(ours, theirs), \
        f"{sql}\nn={n} nulls={nulls}\n{ours[:6]}\nvs\n{theirs[:6]}"


# ------------------------------------------------------------- brute force
def _brute(vals, valid, part, lo, hi, func):
    """fp64 per-row slice loop over rows already sorted by partition."""
    n = len(vals)
    out, ok = [], []
    for i in range(n):
        s = i
        while s > 0 and part[s - 1] == part[i]:
            s -= 1
        e = i
        while e < n - 1 and part[e + 1] == part[i]:
            e += 1
        l = s if lo is None else max(s, i + lo)
        r = e if hi is None else min(e, i + hi)
        rows = list(range(l, r + 1))
        live = [vals[j] for j in rows if valid[j]]
        if func == "count_star":
            res = float(len(rows))
        elif func == "count":
            res = float(len(live))
        elif func == "first_value":
            res = vals[l] if rows and valid[l] else None
        elif func == "last_value":
            res = vals[r] if rows and valid[r] else None
        elif not live:
            res = None
        elif func == "sum":
            res = sum(live)
        elif func == "avg":
            res = sum(live) / len(live)
        else:
            res = min(live) if func == "min" else max(live)
        out.append(res)
        ok.append(res is not None)
    return out, ok


def _random_sorted_input(rng, n, nulls):
    part, p = [], 0
    while len(part) < n:
        part += [p] * rng.choice([1, 1, 2, 3, 5, 8, 13, 40])
        p += 1
    part = part[:n]
    # integer-valued doubles: every sum is exact, so results compare exactly
    vals = [float(rng.randrange(-50, 50)) for _ in range(n)]
    valid = [not (nulls and rng.random() < 0.3) for _ in range(n)]
    return part, vals, valid


# W = 1, W not a power of two, W a power of two, clipped, empty, one-sided
BRUTE_FRAMES = [(0, 0), (-1, -1), (2, 2), (-2, 0), (-1, 1), (-3, 1), (-6, 0),
                (0, 5), (-7, 3), (-3, -1), (1, 4), (5, 9), (-100, 100),
                (None, 0), (None, -2), (None, 3), (0, None), (2, None),
                (-2, None), (None, None)]


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("func", ["sum", "count", "count_star", "avg", "min",
                                  "max", "first_value", "last_value"])
def test_window_frame_vs_brute_force(func, nulls):
    rng = random.Random(zlib.crc32(f"{func}{nulls}".encode()))
    frames = BRUTE_FRAMES + [
        tuple(sorted((rng.randrange(-12, 13), rng.randrange(-12, 13))))
        for _ in range(10)]
    for lo, hi in frames:
        n = rng.choice([1, 2, 31, 97])
        part, vals, valid = _random_sorted_input(rng, n, nulls)
        perm = list(range(n))
        rng.shuffle(perm)
        got, got_ok = ops.window_frame(
            None if func == "count_star"
            else torch.tensor(vals, dtype=torch.float64),
            torch.tensor(valid) if nulls else None,
            torch.tensor(part), lo, hi, func, torch.tensor(perm))
        want, want_ok = _brute(vals, valid, part, lo, hi, func)
        assert got.dtype == torch.float64 and got_ok.dtype == torch.bool
        for i in range(n):
            assert bool(got_ok[perm[i]]) == want_ok[i], (lo, hi, i)
            if want_ok[i]:
                assert float(got[perm[i]]) == pytest.approx(
                    want[i], rel=1e-12, abs=0), (lo, hi, i)


def test_frame_without_order_by_runs_in_input_order():
    rng = random.Random(5)
    n = 60
    k = [rng.randrange(4) for _ in range(n)]
    v = [float(rng.randrange(100)) for _ in range(n)]
    out = SqlExecutor(
        "SELECT max(v) OVER (PARTITION BY k ROWS BETWEEN 2 PRECEDING AND "
        "CURRENT ROW) AS m FROM flow").execute(
            {"flow": MessageBatch.from_dict({"k": k, "v": v})})
    got = out.columns["m"].to_pylist()
    for i in range(n):
        prev = [j for j in range(i + 1) if k[j] == k[i]][-3:]
        assert got[i] == max(v[j] for j in prev)


def test_result_dtypes_and_validity():
    data = {"id": [0, 1, 2, 3], "k": [0, 0, 1, 1],
            "i": [5, None, 7, 8], "f": [1.5, 2.5, None, 4.5]}
    fr = "PARTITION BY k ORDER BY id ROWS BETWEEN 1 PRECEDING AND 1 PRECEDING"
    out = SqlExecutor(
        f"SELECT sum(i) OVER ({fr}) AS s, count(i) OVER ({fr}) AS c, "
        f"count(*) OVER ({fr}) AS n, first_value(i) OVER ({fr}) AS fv, "
        f"last_value(f) OVER ({fr}) AS lv, min(f) OVER ({fr}) AS lo "
        "FROM flow").execute({"flow": MessageBatch.from_dict(data)})
    c = out.columns
    assert c["s"].data.dtype == torch.float64
    assert c["c"].data.dtype == torch.int64 and c["c"].validity is None
    assert c["n"].data.dtype == torch.int64
    assert c["fv"].data.dtype == torch.int64
    assert c["lv"].data.dtype == c["lo"].data.dtype == torch.float64
    assert c["s"].to_pylist() == [None, 5.0, None, 7.0]
    assert c["c"].to_pylist() == [0, 1, 0, 1]
    assert c["n"].to_pylist() == [0, 1, 0, 1]
    assert c["fv"].to_pylist() == [None, 5, None, 7]
    assert c["lv"].to_pylist() == [None, 1.5, None, None]
    assert c["lo"].to_pylist() == [None, 1.5, None, None]


# ----------------------------------------------------------- segmented scan
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("op", ["sum", "min", "max"])
def test_segmented_scan_cpu(op, reverse):
    rng = random.Random(11)
    for n in (0, 1, 2, 33, 200):
        vals = [float(rng.randrange(-9, 10)) for _ in range(n)]
        head = [rng.random() < 0.2 for _ in range(n)]
        got = ops.segmented_scan(torch.tensor(vals, dtype=torch.float64),
                                 torch.tensor(head, dtype=torch.bool), op,
                                 reverse).tolist()
        fn = {"sum": lambda x, y: x + y, "min": min, "max": max}[op]
        order = range(n - 1, -1, -1) if reverse else range(n)
        want, run = [0.0] * n, None
        for i in order:
            run = vals[i] if run is None or head[i] else fn(run, vals[i])
            want[i] = run
        assert got == want


# ------------------------------------------------------------------ parser
def test_frame_is_parsed_into_signed_offsets():
    def frame(clause):
        sel = parse_sql(f"SELECT sum(a) OVER (ORDER BY a {clause}) FROM flow")
        return sel.projections[0][0].over.frame
    assert frame("") is None
    assert frame("ROWS BETWEEN 9 PRECEDING AND CURRENT ROW") == ("rows", -9, 0)
    assert frame("rows between 1 following and 4 following") == ("rows", 1, 4)
    assert frame("ROWS 5 PRECEDING") == ("rows", -5, 0)
    assert frame("ROWS UNBOUNDED PRECEDING") == ("rows", None, 0)
    assert frame("ROWS BETWEEN CURRENT ROW AND UNBOUNDED FOLLOWING") == \
        ("rows", 0, None)
    assert frame("RANGE BETWEEN UNBOUNDED PRECEDING AND UNBOUNDED "
                 "FOLLOWING") == ("range", None, None)
    assert frame("RANGE UNBOUNDED PRECEDING") == ("range", None, 0)


@pytest.mark.parametrize("clause, message", [
    ("ROWS BETWEEN CURRENT ROW AND 1 PRECEDING", "start is after"),
    ("ROWS BETWEEN 1 FOLLOWING AND CURRENT ROW", "start is after"),
    ("ROWS BETWEEN 2 PRECEDING AND 3 PRECEDING", "start is after"),
    ("ROWS 1 FOLLOWING", "start is after"),
    ("ROWS BETWEEN UNBOUNDED FOLLOWING AND UNBOUNDED FOLLOWING",
     "start at UNBOUNDED FOLLOWING"),
    ("ROWS UNBOUNDED FOLLOWING", "start at UNBOUNDED FOLLOWING"),
    ("ROWS BETWEEN UNBOUNDED PRECEDING AND UNBOUNDED PRECEDING",
     "end at UNBOUNDED PRECEDING"),
    ("ROWS BETWEEN -1 PRECEDING AND CURRENT ROW", "non-negative integer"),
    ("ROWS BETWEEN 1.5 PRECEDING AND CURRENT ROW", "non-negative integer"),
    ("ROWS BETWEEN a PRECEDING AND CURRENT ROW", "non-negative integer"),
    ("ROWS 2e1 PRECEDING", "non-negative integer"),
    ("GROUPS BETWEEN 1 PRECEDING AND CURRENT ROW", "GROUPS"),
    ("ROWS BETWEEN 1 PRECEDING AND CURRENT ROW EXCLUDE CURRENT ROW",
     "EXCLUDE"),
    ("ROWS 1 PRECEDING EXCLUDE TIES", "EXCLUDE"),
    ("RANGE BETWEEN 1 PRECEDING AND CURRENT ROW", "RANGE.*numeric offset"),
    ("RANGE BETWEEN UNBOUNDED PRECEDING AND 1 FOLLOWING",
     "RANGE.*numeric offset"),
    ("RANGE 3 PRECEDING", "RANGE.*numeric offset"),
    ("RANGE BETWEEN CURRENT ROW AND UNBOUNDED FOLLOWING",
     "RANGE.*CURRENT ROW"),
    ("RANGE BETWEEN CURRENT ROW AND CURRENT ROW", "RANGE.*CURRENT ROW"),
    ("RANGE CURRENT ROW", "RANGE.*CURRENT ROW"),
    ("ROWS BETWEEN 1 PRECEDING", "expected and"),
    ("ROWS BETWEEN UNBOUNDED AND CURRENT ROW", "PRECEDING or FOLLOWING"),
    ("ROWS 2", "PRECEDING or FOLLOWING"),
    ("ROWS CURRENT", "expected ROW"),
])
def test_frame_errors(clause, message):
    with pytest.raises(SqlError, match=message):
        SqlExecutor(f"SELECT sum(a) OVER (PARTITION BY k ORDER BY a {clause})"
                    " FROM flow")


def test_last_value_needs_a_frame():
    flow = MessageBatch.from_dict({"a": [1, 2, 3]})
    with pytest.raises(SqlError, match="last_value"):
        SqlExecutor("SELECT last_value(a) OVER (ORDER BY a) FROM flow"
                    ).execute({"flow": flow})


def test_frame_words_stay_ordinary_column_names():
    data = {"rows": [3, 1, 2, 5, 4], "row": [0, 1, 2, 3, 4],
            "range": [1, 1, 2, 2, 2], "current": [9, 8, 7, 6, 5],
            "preceding": [1, 2, 3, 4, 5], "following": [5, 4, 3, 2, 1],
            "unbounded": [0, 0, 1, 1, 0]}
    flow = {"flow": MessageBatch.from_dict(data)}

    def run(sql):
        out = SqlExecutor(sql).execute(flow)
        return [tuple(r.values()) for r in out.to_rows()]

    assert run("SELECT rows, row, range FROM flow WHERE rows > 1 AND "
               "range = 2 ORDER BY row DESC") == [(4, 4, 2), (5, 3, 2),
                                                  (2, 2, 2)]
    assert run("SELECT range, sum(rows) AS rows, max(current) AS row "
               "FROM flow GROUP BY range ORDER BY range") == \
        [(1, 4, 9), (2, 11, 7)]
    assert run("SELECT unbounded + preceding * following AS current "
               "FROM flow ORDER BY row") == [(5,), (8,), (10,), (9,), (5,)]
    # inside OVER: as partition key, order key and argument, next to a frame
    assert run("SELECT sum(rows) OVER (PARTITION BY range ORDER BY row ROWS "
               "BETWEEN 1 PRECEDING AND CURRENT ROW) AS s FROM flow "
               "ORDER BY row") == [(3.0,), (4.0,), (2.0,), (7.0,), (9.0,)]
    assert run("SELECT count(*) OVER (PARTITION BY rows) AS c, "
               "min(range) OVER (ORDER BY range) AS m, "
               "row_number() OVER (ORDER BY rows) AS rn FROM flow "
               "ORDER BY row") == [(1, 1.0, 3), (1, 1.0, 1), (1, 1.0, 2),
                                   (1, 1.0, 5), (1, 1.0, 4)]
    assert run("SELECT sum(row) OVER (ORDER BY rows RANGE UNBOUNDED "
               "PRECEDING) AS s FROM flow ORDER BY rows") == \
        [(1.0,), (3.0,), (3.0,), (7.0,), (10.0,)]
