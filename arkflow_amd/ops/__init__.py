"""Physical op dispatch: hand-written HIP kernels on GPU, torch on CPU.

Every hot physical operator of the SQL/inference path routes through here.
On a CUDA(=ROCm) device the native gfx950 extension (arkflow_amd._native,
built from csrc/) is REQUIRED — if it is missing we raise
GpuExtensionMissing instead of silently falling back to eager PyTorch, so a
GPU test can never pass on a non-native path. On CPU, torch reference
implementations keep CI green and serve as the numerics oracle.
"""
from __future__ import annotations
import struct
from typing import Optional, Tuple

import torch

from ..errors import GpuExtensionMissing

_native = None
_native_err: Optional[str] = None


def _load_native():
    global _native, _native_err
    if _native is not None or _native_err is not None:
        return _native
    try:
        from .. import _native as mod  # built in-tree by setup.py build_ext
        _native = mod
    except ImportError as e:
        _native_err = str(e)
    return _native


def native_available() -> bool:
    return _load_native() is not None


def require_native():
    mod = _load_native()
    if mod is None:
        raise GpuExtensionMissing(
            f"arkflow_amd._native HIP extension not built ({_native_err}); "
            "run `python setup.py build_ext --inplace` (gfx950)"
        )
    return mod


def _use_native(t: torch.Tensor) -> bool:
    if t.is_cuda:
        require_native()  # fail loudly on GPU without the extension
        return True
    return False


# --------------------------------------------------------------------- filter
def mask_to_indices(mask: torch.Tensor) -> torch.Tensor:
    """Order-preserving stream compaction: bool[n] → int32 indices of set rows.

    GPU: two-pass block-count + scan + scatter HIP kernel (csrc/filter.hip),
    replacing the reference's DataFusion FilterExec (processor/sql.rs:107).
    """
    if _use_native(mask):
        return require_native().mask_to_indices(mask)
    return torch.nonzero(mask, as_tuple=False).flatten().to(torch.int32)


def filter_cmp_scalar(col: torch.Tensor, op: str, scalar: float) -> torch.Tensor:
    """Fused compare+compact for the common `WHERE col OP literal` shape:
    returns indices directly without materializing the mask."""
    if _use_native(col):
        opi = {"<": 0, "<=": 1, ">": 2, ">=": 3, "=": 4, "!=": 5}[op]
        return require_native().filter_cmp_scalar(col, opi, float(scalar))
    mask = {
        "<": col < scalar, "<=": col <= scalar, ">": col > scalar,
        ">=": col >= scalar, "=": col == scalar, "!=": col != scalar,
    }[op]
    return torch.nonzero(mask, as_tuple=False).flatten().to(torch.int32)


def gather(col: torch.Tensor, indices: torch.Tensor) -> torch.Tensor:
    """Row gather. GPU: coalesced gather kernel handling 1/2/4/8-byte elems."""
    if _use_native(col):
        return require_native().gather(col, indices)
    return col[indices.long()]


# ------------------------------------------------------------------ aggregate
def hash_group(keys: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """Group rows by an integer key column.

    Returns (group_ids int32[n], unique_keys[g], num_groups). GPU: LDS-tiled
    open-addressing hash build (csrc/hash_agg.hip) — replaces DataFusion's
    hash-aggregate physical operator.
    """
    if _use_native(keys):
        gid, uniq = require_native().hash_group_i64(keys.to(torch.int64))
        return gid, uniq, int(uniq.shape[0])
    uniq, inverse = torch.unique(keys, return_inverse=True)
    return inverse.to(torch.int32), uniq, int(uniq.shape[0])


def segment_reduce(values: torch.Tensor, group_ids: torch.Tensor,
                   num_groups: int, op: str) -> torch.Tensor:
    """Per-group reduction: op in sum|min|max|count|mean."""
    gid = group_ids.long()
    if op == "count":
        if values.is_cuda and values.shape[0] < (1 << 24):
            # int64 scatter_add on GPU is a CAS loop — catastrophic under
            # high key contention; the native f32 LDS-buffered sum is exact
            # for counts < 2^24 per group and orders of magnitude faster.
            # No group can hold 2^24 rows when the batch has fewer; a larger
            # batch counts in int64 below.
            ones = torch.ones(values.shape[0], dtype=torch.float32,
                              device=values.device)
            return segment_reduce(ones, group_ids, num_groups,
                                  "sum").to(torch.int64)
        out = torch.zeros(num_groups, dtype=torch.int64, device=values.device)
        out.scatter_add_(0, gid, torch.ones_like(gid))
        return out
    v = values.to(torch.float64) if values.dtype in (
        torch.float16, torch.bfloat16) else values
    if _use_native(values) and op in ("sum", "min", "max") \
            and values.dtype == torch.float32:
        opi = {"sum": 0, "min": 1, "max": 2}[op]
        return require_native().segment_reduce_f32(
            values, group_ids, num_groups, opi)
    if op == "sum":
        out = torch.zeros(num_groups, dtype=v.dtype, device=v.device)
        out.scatter_add_(0, gid, v)
        return out
    if op == "mean":
        s = segment_reduce(values, group_ids, num_groups, "sum")
        c = segment_reduce(values, group_ids, num_groups, "count")
        return s.double() / c.double()
    if op in ("min", "max"):
        init = float("inf") if op == "min" else float("-inf")
        out = torch.full((num_groups,), init, dtype=torch.float64,
                         device=v.device)
        out.scatter_reduce_(0, gid, v.double(), reduce="amin" if op == "min"
                            else "amax", include_self=True)
        return out
    raise ValueError(f"unknown segment op {op!r}")


# ----------------------------------------------------------------------- sort
def sort_indices(key: torch.Tensor, ascending: bool = True) -> torch.Tensor:
    """Stable argsort. GPU: native LSD radix sort (csrc/radix_sort.hip) for
    f32/i64/i32 keys; torch elsewhere."""
    if _use_native(key) and key.dtype in (torch.float32, torch.int64,
                                          torch.int32):
        return require_native().radix_argsort(
            key.contiguous(), not ascending).long()
    return torch.argsort(key, stable=True, descending=not ascending)


# --------------------------------------------------------------- string order
# Order of binary columns: bytewise, unsigned, a proper prefix first — Python's
# bytes order, SQLite's BINARY collation, code-point order for UTF-8.
def _bytes_rows(col) -> list:
    """Every row's bytes, NULL rows included (validity is the caller's)."""
    data = col.data.detach().to("cpu").numpy().tobytes()
    off = col.offsets.detach().to("cpu").tolist()
    return [data[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def _check_binary(col, what: str):
    if getattr(col, "kind", None) != "binary":
        raise TypeError(f"{what} takes a binary Column")


def bytes_rank(col) -> torch.Tensor:
    """Dense rank of a binary column, int64[n]: rank[i] is the number of
    distinct strings smaller than row i, so equal strings share a rank and
    rank order is string order. NULL rows rank by whatever bytes they hold.

    GPU: 7-byte chunk keys refined round by round over the radix argsort
    (csrc/bytes_order.hip), one scalar readback per round. CPU: the plain
    Python reference, sorted(set(rows)).
    """
    _check_binary(col, "bytes_rank")
    if _use_native(col.data):
        return require_native().bytes_rank(col.data.contiguous(),
                                           col.offsets.contiguous())
    rows = _bytes_rows(col)
    order = {v: i for i, v in enumerate(sorted(set(rows)))}
    return torch.tensor([order[v] for v in rows], dtype=torch.int64)


def bytes_compare(col, other) -> torch.Tensor:
    """Three-way compare per row, int8[n] of -1 / 0 / +1: ``col`` against a
    second binary Column of the same length, or against one ``bytes`` value.

    GPU: one thread per row, a word at a time where the two sides share their
    alignment (csrc/bytes_order.hip). CPU: (a > b) - (a < b) over the rows.
    """
    _check_binary(col, "bytes_compare")
    lit = None
    if isinstance(other, (bytes, bytearray)):
        lit = bytes(other)
    else:
        _check_binary(other, "bytes_compare")
        if len(other) != len(col):
            raise ValueError("bytes_compare: columns differ in row count")
    if _use_native(col.data):
        nat = require_native()
        if lit is not None:
            return nat.bytes_compare_lit(col.data.contiguous(),
                                         col.offsets.contiguous(), lit)
        if not other.data.is_cuda:
            raise ValueError("bytes_compare: columns on different devices")
        return nat.bytes_compare_cols(
            col.data.contiguous(), col.offsets.contiguous(),
            other.data.contiguous(), other.offsets.contiguous())
    a = _bytes_rows(col)
    b = [lit] * len(a) if lit is not None else _bytes_rows(other)
    return torch.tensor([(x > y) - (x < y) for x, y in zip(a, b)],
                        dtype=torch.int8)


# --------------------------------------------------------------------- window
_SCAN_OPS ={"sum": 0, "min": 1, "max": 2}
_SCAN_IDENTITY = {"sum": 0.0, "min": float("inf"), "max": float("-inf")}
_WINDOW_FUNCS = {"sum": 0, "count": 1, "avg": 2, "min": 3, "max": 4,
                 "first_value": 5, "last_value": 6, "count_star": 7}


def segmented_scan(values: torch.Tensor, head: torch.Tensor, op: str,
                   reverse: bool = False) -> torch.Tensor:
    """Inclusive scan (op in sum|min|max) that restarts at every row whose
    head flag is set; float64 in and out. With ``reverse`` the scan runs from
    the last row down and a flag marks the first row met in that direction.

    GPU: three-pass tile scan carrying (value, seen-a-head) pairs
    (csrc/window.hip). CPU: log-step doubling over whole tensors, one step
    per power of two up to the longest segment.
    """
    if op not in _SCAN_OPS:
        raise ValueError(f"unknown scan op {op!r}")
    v = values.to(torch.float64).contiguous()
    h = head.to(torch.uint8).contiguous()
    if v.shape != h.shape or v.dim() != 1:
        raise ValueError("values and head must be 1-D and equally long")
    if _use_native(v):
        return require_native().segmented_scan(v, h, _SCAN_OPS[op], reverse)
    if reverse:
        return _segmented_scan_torch(v.flip(0), h.flip(0), op).flip(0)
    return _segmented_scan_torch(v, h, op)


def _segmented_scan_torch(v: torch.Tensor, head: torch.Tensor, op: str
                          ) -> torch.Tensor:
    n = v.shape[0]
    y = v.clone()
    seen = head.bool().clone()
    if n:
        seen[0] = True  # nothing precedes row 0
    fn = {"sum": torch.add, "min": torch.minimum, "max": torch.maximum}[op]
    shift = 1
    # after the step with `shift`, y[i] covers the 2*shift rows ending at i
    # (or back to the nearest head); done once every row has seen a head
    while shift < n and not bool(seen.all()):
        open_ = ~seen[shift:]
        y[shift:] = torch.where(open_, fn(y[:-shift], y[shift:]), y[shift:])
        seen[shift:] |= seen[:-shift].clone()
        shift <<= 1
    return y


def window_frame(values: Optional[torch.Tensor],
                 valid: Optional[torch.Tensor], part_ids: torch.Tensor,
                 lo: Optional[int], hi: Optional[int], func: str,
                 perm: Optional[torch.Tensor] = None
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
    """One window function over ``ROWS BETWEEN lo AND hi`` frames.

    Rows arrive sorted by (partition, order key): ``values`` (None for
    count_star) and ``valid`` (None = no NULL input) are per row, ``part_ids``
    are the sorted partition ids. ``lo``/``hi`` are signed row offsets from
    the current row, None = unbounded. func: sum|count|avg|min|max|
    first_value|last_value|count_star. Returns (float64 result, bool valid);
    both go to row ``perm[i]`` when ``perm`` is given, else stay sorted.

    GPU: segmented scans + one frame kernel (csrc/window.hip). CPU: the same
    scheme in torch — prefix differences for sum/count/avg, two scans over
    chunks of the frame width for a sliding min/max.
    """
    if func not in _WINDOW_FUNCS:
        raise ValueError(f"unknown window function {func!r}")
    if lo is not None and hi is not None and lo > hi:
        raise ValueError("frame start is after frame end")
    n = part_ids.shape[0]
    device = part_ids.device
    if values is None:
        values = torch.zeros(n, dtype=torch.float64, device=device)
    v = values.to(torch.float64).contiguous()
    if _use_native(part_ids):
        out, ok = require_native().window_frame(
            v, None if valid is None else valid.to(torch.uint8).contiguous(),
            part_ids.to(torch.int64).contiguous(), lo, hi,
            _WINDOW_FUNCS[func],
            None if perm is None else perm.to(torch.int64).contiguous())
        return out, ok.bool()
    out, ok = _window_frame_torch(v, valid, part_ids, lo, hi, func)
    if perm is not None:
        p = perm.long()
        out = torch.empty_like(out).index_copy_(0, p, out)
        ok = torch.empty_like(ok).index_copy_(0, p, ok)
    return out, ok


def _window_frame_torch(v, valid, part, lo, hi, func):
    n = part.shape[0]
    device = part.device
    if n == 0:
        return (torch.empty(0, dtype=torch.float64, device=device),
                torch.empty(0, dtype=torch.bool, device=device))
    ar = torch.arange(n, dtype=torch.int64, device=device)
    head = torch.ones(n, dtype=torch.bool, device=device)
    head[1:] = part[1:] != part[:-1]
    tail = torch.ones(n, dtype=torch.bool, device=device)
    tail[:-1] = head[1:]
    inf = float("inf")
    start = segmented_scan(torch.where(head, ar, 0).double(), head,
                           "max").long()
    end = segmented_scan(torch.where(tail, ar.double(), inf), tail, "min",
                         reverse=True).long()
    # an offset of n rows already leaves every partition
    l = start if lo is None else torch.maximum(start, ar + max(-n, min(n, lo)))
    r = end if hi is None else torch.minimum(end, ar + max(-n, min(n, hi)))
    empty = l > r
    lc, rc = l.clamp(0, n - 1), r.clamp(0, n - 1)  # gather-safe when empty
    at_start = l == start
    before = (l - 1).clamp(0, n - 1)

    def prefix_diff(p):
        return p[rc] - torch.where(at_start, torch.zeros_like(p), p[before])

    rows = (r - l + 1).clamp(min=0).double()
    if valid is None:
        cnt = rows
    else:
        cnt = torch.where(empty, torch.zeros_like(rows), prefix_diff(
            segmented_scan(valid.double(), head, "sum")))
    some = cnt > 0
    if func == "count_star":
        return rows, torch.ones_like(empty)
    if func == "count":
        return cnt, torch.ones_like(empty)
    if func in ("first_value", "last_value"):
        at = lc if func == "first_value" else rc
        ok = ~empty if valid is None else ~empty & valid.bool()[at]
        return torch.where(ok, v[at], torch.zeros_like(v)), ok
    fill = _SCAN_IDENTITY["sum" if func in ("sum", "avg") else func]
    masked = v if valid is None else torch.where(
        valid.bool(), v, torch.full_like(v, fill))
    if func in ("sum", "avg"):
        res = prefix_diff(segmented_scan(masked, head, "sum"))
        if func == "avg":
            res = res / cnt.clamp(min=1)
    elif lo is None:
        res = segmented_scan(masked, head, func)[rc]
    elif hi is None:
        res = segmented_scan(masked, tail, func, reverse=True)[lc]
    else:
        # sliding min/max (van Herk/Gil-Werman): chunks of w rows from the
        # partition start; a frame spans at most two of them
        w = max(-n, min(n, hi)) - max(-n, min(n, lo)) + 1
        pos = (ar - start) % w
        prefix = segmented_scan(masked, pos == 0, func)
        suffix = segmented_scan(masked, (pos == w - 1) | tail, func,
                                reverse=True)
        fn = torch.minimum if func == "min" else torch.maximum
        same = (lc - start) // w == (rc - start) // w
        res = torch.where(
            same, torch.where((lc - start) % w == 0, prefix[rc], suffix[lc]),
            fn(suffix[lc], prefix[rc]))
    return torch.where(some, res, torch.zeros_like(res)), some


# ------------------------------------------------------------ protobuf encode
def proto_encode(batch_or_columns, schema, prefix: bytes = b""):
    """Encode each row as one scalar proto3 message of ``schema``: a
    MessageBatch or a name → Column dict in, a binary Column on the inputs'
    device out. ``prefix`` (at most 8 bytes, e.g. a schema-registry header)
    opens every row. Columns are matched to fields by name; a field with no
    column is absent, a NULL is absent, proto3 defaults are elided, and a
    value its field cannot hold (fixed32/sfixed32 out of range, a finite
    value beyond float32) raises ProcessError.

    GPU: size pass + offsets scan + write pass + wave-per-row payload copy
    (csrc/proto_encode.hip), one [total_bytes, error] readback. Integer fields
    read their column cast to int64 (floats truncate toward zero), float
    fields cast to float64; a ``string`` field's bytes are copied unchecked.
    CPU, or an input the kernel does not take (see
    protobuf_proc.encode_device): proto_wire.encode_message row by row, which
    the GPU path matches byte for byte on valid UTF-8.
    """
    from ..batch import Column, MessageBatch
    from ..errors import ProcessError
    from ..processors.protobuf_proc import encode_device, encode_rows_host
    prefix = bytes(prefix)
    if len(prefix) > 8:
        raise ValueError("proto_encode prefix is at most 8 bytes")
    batch = batch_or_columns if isinstance(batch_or_columns, MessageBatch) \
        else MessageBatch(dict(batch_or_columns))
    plan = encode_device(schema, batch.columns)
    if plan is None:
        try:
            rows = encode_rows_host(batch, schema)
        except (OverflowError, ValueError, TypeError, struct.error) as e:
            raise ProcessError(f"protobuf encode error: {e}") from e
        return Column.from_bytes([prefix + r for r in rows]).to(batch.device)
    spec, device = plan
    n = batch.num_rows
    cols = batch.columns

    def widen(names, dtype):
        rows = []
        for name in names:
            d = cols[name].data
            if dtype is torch.float64 and d.dtype in (torch.bfloat16,
                                                      torch.float16):
                d = d.to(torch.float32)
            rows.append(d.to(dtype))
        if not rows:
            return torch.empty((0, n), dtype=dtype, device=device)
        return torch.stack(rows).contiguous()

    valids, valid_idx = [], []
    for name in spec.names:
        v = cols[name].validity
        valid_idx.append(-1 if v is None else len(valids))
        if v is not None:
            valids.append(v.to(torch.uint8).contiguous())
    strings = [(cols[name].data.contiguous(), cols[name].offsets.contiguous())
               for name in spec.str_fields]
    data, offsets, summary = require_native().proto_encode(
        widen(spec.int_fields, torch.int64),
        widen(spec.float_fields, torch.float64), strings, spec.fno,
        spec.kind, spec.slot, valids, valid_idx, prefix)
    if int(summary[1]) != 0:
        raise ProcessError(
            "protobuf encode error: a value does not fit its field (fixed32 "
            "/ sfixed32 out of range, float32 overflow) or a row exceeds "
            "2 GiB")
    return Column("binary", data, offsets)


# ----------------------------------------------------------------------- join
def join_inner(left_keys: torch.Tensor, right_keys: torch.Tensor
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Inner equi-join: returns (left_idx, right_idx) pairs.

    GPU: build/probe hash-join kernel (csrc/hash_join.hip). CPU fallback:
    sort-merge via searchsorted (handles duplicate keys on both sides).
    The kernel hashes int64 keys: floating-point keys are refused there
    (TypeError) rather than truncated — encode them to integer ids first.
    """
    if _use_native(left_keys):
        if left_keys.dtype.is_floating_point \
                or right_keys.dtype.is_floating_point:
            raise TypeError(
                "join_inner on a device takes integer keys, got "
                f"{left_keys.dtype} and {right_keys.dtype}")
        return require_native().join_inner_i64(
            left_keys.to(torch.int64), right_keys.to(torch.int64))
    return _join_sort_merge(left_keys, right_keys)


def _join_sort_merge(lk: torch.Tensor, rk: torch.Tensor):
    r_sorted, r_order = torch.sort(rk, stable=True)
    lo = torch.searchsorted(r_sorted, lk, side="left")
    hi = torch.searchsorted(r_sorted, lk, side="right")
    counts = (hi - lo).clamp(min=0)
    total = int(counts.sum().item())
    if total == 0:
        e = torch.empty(0, dtype=torch.int64, device=lk.device)
        return e, e.clone()
    l_idx = torch.repeat_interleave(
        torch.arange(lk.shape[0], device=lk.device), counts)
    offs = torch.repeat_interleave(lo, counts)
    within = torch.arange(total, device=lk.device) - torch.repeat_interleave(
        torch.cumsum(counts, 0) - counts, counts)
    r_idx = r_order[offs + within]
    return l_idx, r_idx


def join_left(left_keys: torch.Tensor, right_keys: torch.Tensor
              ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Left join: right_idx is -1 for unmatched left rows."""
    l_idx, r_idx = join_inner(left_keys, right_keys)
    matched = torch.zeros(left_keys.shape[0], dtype=torch.bool,
                          device=left_keys.device)
    matched[l_idx] = True
    un = torch.nonzero(~matched).flatten()
    l_all = torch.cat([l_idx, un])
    r_all = torch.cat([r_idx, torch.full_like(un, -1)])
    order = torch.argsort(l_all, stable=True)
    return l_all[order], r_all[order]
