"""GPU tests of csrc/window.hip: the segmented scan against an fp64 host loop
at every tile edge, and ROWS-frame SQL on the device against the CPU
executor."""
import itertools
import operator
import random

import pytest
import torch

from arkflow_amd.batch import Column, MessageBatch
from arkflow_amd.sql.engine import SqlExecutor

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def nat():
    from arkflow_amd import ops
    return ops.require_native()  # GPU present ⇒ extension must load


# ----------------------------------------------------------- segmented scan
TILE = 1024          # rows per tile of the scan (checked against the op)
CARRY_BLOCK = 256    # tiles the carry pass scans per loop iteration
SCAN_OPS = {"sum": (0, operator.add), "min": (1, min), "max": (2, max)}


def _host_scan(vals, head, fn, reverse):
    """Sequential fp64 scan, restarted at every head, in scan order."""
    if reverse:
        vals, head = vals[::-1], head[::-1]
    n = len(vals)
    starts = [0] + [i for i in range(1, n) if head[i]]
    out = []
    for s, e in zip(starts, starts[1:] + [n]):
        out.extend(itertools.accumulate(vals[s:e], fn))
    return out[::-1] if reverse else out


def _longest_segment(head, reverse):
    if reverse:
        head = head[::-1]
    n = len(head)
    starts = [0] + [i for i in range(1, n) if head[i]]
    return max(e - s for s, e in zip(starts, starts[1:] + [n]))


def _head_patterns(n, rng):
    """name → head flags. Tile edges are marked from both ends of the array,
    so they fall on tile edges of the forward and of the reverse scan."""
    first = [i == 0 for i in range(n)]
    edges = [False] * n
    for k in range(0, n, TILE):
        for p in (k, k + TILE - 1, n - 1 - k, n - k - TILE):
            if 0 <= p < n:
                edges[p] = True
    # sparse random heads with a gap of 3 tiles: one segment covers more
    # than two whole tiles, so a tile without any head receives a carry
    gap_lo, gap_hi = TILE // 2, 3 * TILE + TILE // 2
    span = [rng.random() < 0.01 and not gap_lo < i < gap_hi
            for i in range(n)]
    return {"none": [False] * n, "first": first, "every": [True] * n,
            "edges": edges, "span": span}


SCAN_SHAPES = [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 5,
               (CARRY_BLOCK + 1) * TILE + 7]  # last: the carry pass loops


@pytest.mark.parametrize("n", SCAN_SHAPES)
def test_segmented_scan(nat, dev, n):
    assert nat.seg_scan_tile_rows() == TILE
    rng = random.Random(n)
    vals = [rng.gauss(0.0, 10.0) for _ in range(n)]
    vmax = max(abs(v) for v in vals)
    dvals = torch.tensor(vals, dtype=torch.float64, device=dev)
    patterns = _head_patterns(n, rng)
    if n > 4 * TILE:  # the large shape is about the carry loop only
        patterns = {k: patterns[k] for k in ("none", "span")}
    for pname, head in patterns.items():
        dhead = torch.tensor(head, dtype=torch.uint8, device=dev)
        for opname, (opi, fn) in SCAN_OPS.items():
            for reverse in (False, True):
                got = nat.segmented_scan(dvals, dhead, opi, reverse).cpu()
                want = torch.tensor(_host_scan(vals, head, fn, reverse),
                                    dtype=torch.float64)
                what = f"n={n} heads={pname} op={opname} reverse={reverse}"
                if opname == "sum":
                    # fp64 reassociation error and nothing else
                    bound = 4 * _longest_segment(head, reverse) * vmax * EPS
                    err = float((got - want).abs().max())
                    print(f"{what}: err {err:.3e} bound {bound:.3e}")
                    assert err <= bound, what
                else:
                    assert torch.equal(got, want), what


def test_segmented_scan_through_ops(dev):
    """The public op: any float dtype and bool heads in, float64 out."""
    from arkflow_amd import ops
    v = torch.arange(1, 11, dtype=torch.float32, device=dev)
    h = torch.zeros(10, dtype=torch.bool, device=dev)
    h[4] = True
    got = ops.segmented_scan(v, h, "sum")
    assert got.is_cuda and got.dtype == torch.float64
    assert got.tolist() == [1, 3, 6, 10, 5, 11, 18, 26, 35, 45]
    # in reverse the flagged row is the first of its segment: rows 4..0
    got = ops.segmented_scan(v, h, "max", reverse=True)
    assert got.tolist() == [5, 5, 5, 5, 5, 10, 10, 10, 10, 10]
    got = ops.segmented_scan(v, h, "min", reverse=True)
    assert got.tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 9, 10]
    assert ops.segmented_scan(v[:0], h[:0], "min").shape == (0,)


# ------------------------------------------------------------ SQL on device
FRAMES = {
    "w1": "ROWS BETWEEN CURRENT ROW AND CURRENT ROW",
    "w7": "ROWS BETWEEN 3 PRECEDING AND 3 FOLLOWING",
    "w_over_tile": "ROWS BETWEEN 1500 PRECEDING AND CURRENT ROW",
    "w_over_partitions": "ROWS BETWEEN 5000 PRECEDING AND 5000 FOLLOWING",
    "empty": "ROWS BETWEEN 3 PRECEDING AND 1 PRECEDING",
    "running": "ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW",
    "to_end": "ROWS BETWEEN 2 FOLLOWING AND UNBOUNDED FOLLOWING",
}
FUNCS = ["sum", "count", "avg", "min", "max", "first_value", "last_value"]
# partitions from one row to more than two tiles, about 20 000 rows in all
PART_SIZES = [1, 1, 2, 3, 7, 63, 64, 65, 700, TILE - 1, TILE, TILE + 1,
              2 * TILE + 452, 3000, 3333, 4000, 2900]


@pytest.fixture(scope="module")
def flow():
    """(cpu batch, longest partition, max |v|) per nulls flag; rows shuffled,
    id a unique order key."""
    out = {}
    for nulls in (False, True):
        g = torch.Generator().manual_seed(7 + nulls)
        k = torch.cat([torch.full((s,), 1000 + 3 * i, dtype=torch.int64)
                       for i, s in enumerate(PART_SIZES)])
        n = k.shape[0]
        k = k[torch.randperm(n, generator=g)]
        v = torch.randn(n, generator=g) * 10
        cols = {"k": Column("numeric", k),
                "id": Column("numeric", torch.randperm(n, generator=g)),
                "v": Column("numeric", v)}
        if nulls:
            cols["v"].validity = torch.rand(n, generator=g) >= 0.3
        out[nulls] = (MessageBatch(cols), max(PART_SIZES),
                      float(v.abs().max()))
    return out


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("frame", list(FRAMES))
def test_sql_frames_on_device(nat, dev, flow, frame, nulls):
    batch, longest, vmax = flow[nulls]
    over = f"OVER (PARTITION BY k ORDER BY id {FRAMES[frame]})"
    sql = "SELECT " + ", ".join(f"{f}(v) {over} AS {f}" for f in FUNCS) \
        + f", count(*) {over} AS count_star FROM flow"
    ex = SqlExecutor(sql)
    want = ex.execute({"flow": batch})
    got = ex.execute({"flow": batch.to(dev)})
    bound = 4 * longest * vmax * EPS
    for name in FUNCS + ["count_star"]:
        g, w = got.columns[name], want.columns[name]
        assert g.data.is_cuda, name
        assert g.data.dtype == w.data.dtype, name
        assert (g.validity is None) == (w.validity is None), name
        gd, wd = g.data.cpu(), w.data
        if w.validity is not None:
            assert g.validity.is_cuda, name
            assert torch.equal(g.validity.cpu(), w.validity), name
            gd, wd = gd[w.validity], wd[w.validity]
        if name in ("sum", "avg"):
            err = float((gd - wd).abs().max()) if len(gd) else 0.0
            print(f"{frame} nulls={nulls} {name}: err {err:.3e} "
                  f"bound {bound:.3e}")
            assert err <= bound, name
        else:
            assert torch.equal(gd, wd), name
