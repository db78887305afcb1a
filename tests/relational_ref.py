"""Host-side references and key sets for the relational kernel tests (radix
argsort, hash GROUP BY, hash join, segment reduce). Everything here runs on
the CPU in int64 / fp64; nothing touches a device."""
import collections

import numpy as np
import torch

I64_MIN = -(1 << 63)
I64_MAX = (1 << 63) - 1
# around the 64-lane wave and the 4096-row tile of a radix pass
SORT_SIZES = (1, 63, 64, 65, 255, 4095, 4096, 4097, 8191, 8193,
              3 * 4096 + 1)
U24 = 2.0 ** -24   # unit roundoff of f32


# ----------------------------------------------------------------- hashing
def mix64(z):
    """common.h mix64 on a numpy uint64 array (or one Python int)."""
    scalar = not isinstance(z, np.ndarray)
    z = np.atleast_1d(np.asarray(z, dtype=np.int64)).view(np.uint64).copy()
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xbf58476d1ce4e5b9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94d049bb133111eb)
        z ^= z >> np.uint64(31)
    return int(z[0]) if scalar else z


def table_size(n):
    """Slots of the open-addressing table built for n rows."""
    want = max(2 * n, 64)
    size = 1
    while size < want:
        size <<= 1
    return size


def wrap_cluster(n, cluster=32):
    """Keys for an n-row table whose linear probing must wrap to slot 0.

    Returns (build, miss_inside, miss_past), int64 tensors:
      build        min(n, cluster) keys whose home slot is one of the last two
                   of the table, padded to n rows with keys homed elsewhere in
                   the middle of the table (n rows, all distinct);
      miss_inside  keys homed on the last two slots that are not in build;
      miss_past    keys not in build homed on the first slots, where the
                   wrapped cluster lies and just past its end.
    """
    mask = table_size(n) - 1
    c = min(n, cluster)
    span = 1 << 15
    while True:
        cand = np.arange(-span, span, dtype=np.int64)
        home = mix64(cand) & np.uint64(mask)
        tail = cand[home >= np.uint64(mask - 1)]
        head = cand[home <= np.uint64(c + 1)]
        if len(tail) >= c + 8 and len(head) >= 8:
            break
        span <<= 1
    rng = np.random.default_rng(n)
    tail = rng.permutation(tail)
    build = tail[:c]
    # filler homed in the middle half of the table: it cannot touch the
    # cluster, whatever order the rows are inserted in
    lo, hi = np.uint64(mask // 4), np.uint64(3 * (mask // 4))
    mid = cand[(home >= lo) & (home < hi)]
    assert len(mid) >= n - c
    filler = rng.permutation(mid)[:n - c]
    build = rng.permutation(np.concatenate([build, filler]))
    assert len(np.unique(build)) == n
    return (torch.from_numpy(build), torch.from_numpy(tail[c:c + 8].copy()),
            torch.from_numpy(rng.permutation(head)[:8].copy()))


# -------------------------------------------------------------------- keys
F32_SPECIAL_BITS = (
    0x7f800000, 0xff800000,              # +inf, -inf
    0x7f7fffff, 0xff7fffff,              # largest normals
    0x00800000, 0x80800000,              # smallest normals
    0x00000001, 0x80000001, 0x007fffff, 0x807fffff,  # denormals
    0x00000000, 0x80000000, 0x00000000, 0x80000000,  # +0 / -0 interleaved
    0x80000000, 0x00000000,
    0x7fc00000, 0xffc00000,              # quiet NaN, both signs
    0x7f800001, 0xff800001,              # signalling NaN, low payload
    0x7fffffff, 0xffffffff, 0x7fc12345, 0xffc54321,  # other payloads
    0x3f800000, 0xbf800000,              # 1.0, -1.0
)


def _from_bits32(bits, dtype):
    a = np.asarray(bits, dtype=np.uint64).astype(np.uint32)
    return torch.from_numpy(a.view(np.int32).copy()).view(dtype)


def _random_bits(gen, n, dtype):
    nbytes = torch.empty(0, dtype=dtype).element_size()
    raw = torch.randint(0, 256, (n, nbytes), generator=gen, dtype=torch.uint8)
    return raw.view(dtype).reshape(n)


def sort_key_sets(n, dtype, seed):
    """(name, keys) pairs of n host keys of the given dtype."""
    gen = torch.Generator().manual_seed(seed)
    nbytes = torch.empty(0, dtype=dtype).element_size()
    int_t = torch.int32 if nbytes == 4 else torch.int64
    sets = []

    one = _random_bits(gen, 1, dtype)
    if dtype == torch.float32:
        one = torch.tensor([-2.5])
    sets.append(("all_equal", one.repeat(n)))

    two = torch.tensor([7, -3], dtype=int_t).to(dtype)
    sets.append(("two_values", two[torch.randint(0, 2, (n,), generator=gen)]))

    # 256 values that differ in one byte only: that pass does all the work
    # and every other pass sees a single bin
    base = 0x0012345600123456 & ((1 << (8 * nbytes)) - 1)
    for pos in range(nbytes):
        vals = [(base & ~(0xff << (8 * pos))) | (b << (8 * pos))
                for b in range(256)]
        arr = np.asarray(vals, dtype=np.uint64)
        arr = arr.astype(np.uint32).view(np.int32) if nbytes == 4 \
            else arr.view(np.int64)
        vals_t = torch.from_numpy(arr.copy()).view(dtype)
        pick = torch.randint(0, 256, (n,), generator=gen)
        if n >= 256:  # every value present
            pick[torch.randperm(n, generator=gen)[:256]] = torch.arange(256)
        sets.append((f"byte{pos}", vals_t[pick]))

    full = _random_bits(gen, n, dtype)
    if dtype != torch.float32:
        info = torch.iinfo(dtype)
        full[0] = info.min
        full[-1] = info.max if n > 1 else info.min
        if n > 4:
            full[n // 2] = info.max
            full[n // 2 + 1] = info.min
    sets.append(("full_range", full))

    if dtype == torch.float32:
        spec = _from_bits32(F32_SPECIAL_BITS, torch.float32)
        sets.append(("f32_special",
                     spec[torch.randint(0, len(spec), (n,), generator=gen)]
                     if n < len(spec) else
                     torch.cat([spec, spec[torch.randint(
                         0, len(spec), (n - len(spec),), generator=gen)]])))
    return sets


def limit_keys_mixture(n, seed):
    """int64 keys: INT64_MIN, INT64_MAX, 0, -1 mixed with random keys."""
    gen = torch.Generator().manual_seed(seed)
    lim = torch.tensor([I64_MIN, I64_MAX, 0, -1, I64_MIN + 1, I64_MAX - 1])
    rnd = torch.randint(-40, 40, (n,), generator=gen)
    pick = torch.randint(0, 2 * len(lim), (n,), generator=gen)
    keys = torch.where(pick < len(lim), lim[pick % len(lim)], rnd)
    keys[:min(n, len(lim))] = lim[:min(n, len(lim))]
    return keys[torch.randperm(n, generator=gen)]


# --------------------------------------------------------------- references
def join_pairs(lk, rk):
    """Exact inner-join pair set of two host key tensors, as an int64 [m, 2]
    tensor sorted lexicographically by (left, right)."""
    rows = collections.defaultdict(list)
    for j, k in enumerate(rk.tolist()):
        rows[k].append(j)
    pairs = [(i, j) for i, k in enumerate(lk.tolist()) for j in rows.get(k, ())]
    return torch.tensor(pairs, dtype=torch.int64).reshape(-1, 2)


def left_join_pairs(lk, rk):
    """Same for a left join: an unmatched left row pairs with -1."""
    rows = collections.defaultdict(list)
    for j, k in enumerate(rk.tolist()):
        rows[k].append(j)
    pairs = []
    for i, k in enumerate(lk.tolist()):
        pairs.extend((i, j) for j in rows.get(k, (-1,)))
    return torch.tensor(pairs, dtype=torch.int64).reshape(-1, 2)


def sorted_pairs(l_idx, r_idx):
    """Device result -> host [m, 2] tensor in the order of join_pairs."""
    p = torch.stack([l_idx.cpu().long(), r_idx.cpu().long()], dim=1)
    p = p[torch.argsort(p[:, 1], stable=True)]
    return p[torch.argsort(p[:, 0], stable=True)]


def segment_ref(vals, gids, g):
    """fp64 references of a segment reduction over host tensors.

    Returns (sum, min, max, rows, abs_sum), all float64[g] except rows
    (int64). Empty groups hold 0, +inf, -inf. NaN propagates into min / max
    of its group."""
    v = vals.double()
    gi = gids.long()
    s = torch.zeros(g, dtype=torch.float64).index_add_(0, gi, v)
    a = torch.zeros(g, dtype=torch.float64).index_add_(0, gi, v.abs())
    rows = torch.zeros(g, dtype=torch.int64).index_add_(
        0, gi, torch.ones_like(gi))
    mn = torch.full((g,), float("inf"), dtype=torch.float64)
    mn.scatter_reduce_(0, gi, v, "amin", include_self=True)
    mx = torch.full((g,), float("-inf"), dtype=torch.float64)
    mx.scatter_reduce_(0, gi, v, "amax", include_self=True)
    return s, mn, mx, rows, a


def sum_bound(rows, abs_sum):
    """|f32 sum - exact| <= n_g * 2^-23 * sum|v| for ANY summation order:
    the first-order bound is (n_g - 1) * 2^-24 * sum|v|; the doubling covers
    the higher-order terms and the two-level (LDS, then global) order."""
    return rows.double() * (2 * U24) * abs_sum


def f32_index_order_sum(vals, gids, g):
    """f32 accumulation in row order on the host: the plainest kernel the
    bound must admit."""
    out = np.zeros(g, dtype=np.float32)
    np.add.at(out, gids.long().numpy(), vals.numpy().astype(np.float32))
    return torch.from_numpy(out).double()


def spread_values(n, gen):
    """Mixed signs, magnitudes log-uniform over 1e-3 .. 1e3."""
    mag = 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 6 - 3)
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    return (mag * sign).float()
