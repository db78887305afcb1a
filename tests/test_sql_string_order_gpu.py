"""String order in the SQL executor on a device batch. Three kinds of check:
the device executor against the CPU executor on the queries of
test_sql_string_order.py (which SQLite validates there), window functions
ordered by a string key against a plain Python reference, and that none of the
non-window queries materialises rows on the host: Column.to_pylist and
Column.to_strlist raise while the device query runs. All comparisons are
exact; the sums are of small integers."""
import pytest
import torch

from arkflow_amd import ops
from arkflow_amd.batch import Column
from arkflow_amd.sql.engine import SqlExecutor
from test_sql_string_order import QUERIES, make_batch, make_table, rows_of

pytestmark = pytest.mark.gpu

N = 2000
# stability on equal strings shows only with a column that tells ties apart
DEVICE_QUERIES = QUERIES + [
    ("SELECT id, s FROM flow ORDER BY s", True),
    ("SELECT * FROM flow ORDER BY s1 DESC, s2", True),
    ("SELECT id, s FROM flow ORDER BY s NULLS LAST LIMIT 50", True),
    ("SELECT s1, min(s2), max(u), count(*) FROM flow GROUP BY s1", False),
    ("SELECT id FROM flow WHERE s NOT BETWEEN 'b' AND 'q'", False),
    ("SELECT id FROM flow WHERE s1 < s2 OR s <= 'device-0100'", False),
]
_TABLES = {}
_CPU_ROWS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    ops.require_native()
    return torch.device("cuda:0")


def _tables(nulls, dev):
    """(python lists, CPU batch, device batch) of one variant, built once."""
    if nulls not in _TABLES:
        data = make_table(77 + nulls, N, nulls)
        batch = make_batch(data)
        _TABLES[nulls] = (data, batch, batch.to(dev))
    return _TABLES[nulls]


def _cpu_rows(sql, nulls, dev):
    if (sql, nulls) not in _CPU_ROWS:
        _, batch, _ = _tables(nulls, dev)
        _CPU_ROWS[sql, nulls] = rows_of(
            SqlExecutor(sql).execute({"flow": batch}))
    return _CPU_ROWS[sql, nulls]


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("qi", range(len(DEVICE_QUERIES)))
def test_device_vs_cpu_executor(dev, qi, nulls):
    sql, ordered = DEVICE_QUERIES[qi]
    _, _, on_dev = _tables(nulls, dev)
    out = SqlExecutor(sql).execute({"flow": on_dev})
    assert out.device.type == "cuda"
    got, want = rows_of(out), _cpu_rows(sql, nulls, dev)
    if not ordered:
        got, want = sorted(got, key=repr), sorted(want, key=repr)
    assert got == want, f"{sql}\n{got[:6]}\nvs\n{want[:6]}"


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("qi", range(len(QUERIES)))
def test_no_host_row_materialisation(dev, monkeypatch, qi, nulls):
    sql, ordered = QUERIES[qi]
    _, _, on_dev = _tables(nulls, dev)

    def refuse(self):
        raise AssertionError("rows materialised on the host")

    with monkeypatch.context() as m:
        m.setattr(Column, "to_pylist", refuse)
        m.setattr(Column, "to_strlist", refuse)
        out = SqlExecutor(sql).execute({"flow": on_dev})
    got, want = rows_of(out), _cpu_rows(sql, nulls, dev)
    if not ordered:
        got, want = sorted(got, key=repr), sorted(want, key=repr)
    assert got == want


# ------------------------------------------------- windows, Python reference
def _skey(s):
    """NULL sorts before every string, as for numeric window keys."""
    return (s is not None, (s or "").encode())


def _ref_row_number(d):
    out = {}
    for g in set(d["k"]):
        rows = sorted((i for i in range(N) if d["k"][i] == g),
                      key=lambda i: (_skey(d["s"][i]), d["id"][i]))
        for rn, i in enumerate(rows, 1):
            out[d["id"][i]] = rn
    return [(i, out[i]) for i in sorted(out)]


def _ref_running_sum(d):
    """RANGE UNBOUNDED PRECEDING .. CURRENT ROW: every peer of a tie gets
    the sum through the whole tie."""
    totals = {}
    for i in range(N):
        key = (d["k"][i], _skey(d["s"][i]))
        totals[key] = totals.get(key, 0) + d["x"][i]
    out = {}
    for i in range(N):
        g, sk = d["k"][i], _skey(d["s"][i])
        out[d["id"][i]] = sum(t for (g2, sk2), t in totals.items()
                              if g2 == g and sk2 <= sk)
    return [(i, out[i]) for i in sorted(out)]


def _ref_frame_sum(d):
    rows = sorted(range(N), key=lambda i: d["u"][i].encode())
    out = {}
    for j, i in enumerate(rows):
        out[d["id"][i]] = d["x"][i] + (d["x"][rows[j - 1]] if j else 0)
    return [(i, out[i]) for i in sorted(out)]


WINDOWS = [
    ("SELECT id, row_number() OVER (PARTITION BY k ORDER BY s, id) AS rn "
     "FROM flow ORDER BY id", _ref_row_number),
    ("SELECT id, sum(x) OVER (PARTITION BY k ORDER BY s) AS rs FROM flow "
     "ORDER BY id", _ref_running_sum),
    ("SELECT id, sum(x) OVER (ORDER BY u ROWS BETWEEN 1 PRECEDING AND "
     "CURRENT ROW) AS fs FROM flow ORDER BY id", _ref_frame_sum),
]


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("wi", range(len(WINDOWS)))
def test_window_string_key_vs_python(dev, wi, nulls):
    sql, ref = WINDOWS[wi]
    data, _, on_dev = _tables(nulls, dev)
    out = SqlExecutor(sql).execute({"flow": on_dev})
    assert rows_of(out) == ref(data)
