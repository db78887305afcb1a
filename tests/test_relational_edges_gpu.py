"""Relational kernels (radix argsort, hash GROUP BY, hash join, segment
reduce) against exact host references, at the keys and sizes where such
kernels go wrong: tile and wave edges, every digit pass, the int64 limits
(INT64_MIN is also the tables' free-slot marker), probe sequences that wrap
the table end, signed zeros and NaNs.

Every expected value is computed on the CPU from a host copy of the inputs,
in int64 or fp64 (tests/relational_ref.py); no GPU op serves as reference.
"""
import pytest
import torch

from tests import relational_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def nat():
    from arkflow_amd import ops
    return ops.require_native()


# ------------------------------------------------------------- radix argsort
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.int32, torch.int64])
def test_radix_argsort_exact_permutation(nat, dev, dtype, descending):
    """The result is THE stable permutation, index for index: sorted values
    alone would pass a sort that is unstable or, with duplicate keys, one
    that is not a permutation at all."""
    for n in R.SORT_SIZES:
        for name, keys in R.sort_key_sets(n, dtype, seed=n):
            exp = torch.argsort(keys, stable=True, descending=descending)
            got = nat.radix_argsort(keys.to(dev), descending).cpu().long()
            assert torch.equal(got, exp), \
                f"{dtype} n={n} {name} descending={descending}"


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32, torch.int64])
def test_sort_indices_matches_host(dev, dtype):
    from arkflow_amd import ops
    for n in (65, 4097):
        for name, keys in R.sort_key_sets(n, dtype, seed=100 + n):
            for asc in (True, False):
                exp = torch.argsort(keys, stable=True, descending=not asc)
                got = ops.sort_indices(keys.to(dev), ascending=asc)
                assert got.dtype == torch.int64
                assert torch.equal(got.cpu(), exp), f"{dtype} n={n} {name}"


def test_sort_chain_two_keys_matches_host(dev):
    """ORDER BY A, B the way the engine runs it: sort by B, then stably by A.
    A holds +0.0, -0.0 and duplicates; a sort that orders -0.0 before +0.0
    breaks the B order inside the zeros."""
    from arkflow_amd import ops
    gen = torch.Generator().manual_seed(11)
    n = 4097
    a_vals = torch.tensor([0.0, -0.0, 1.5, -1.5, 0.0, -0.0, float("inf")])
    a = a_vals[torch.randint(0, len(a_vals), (n,), generator=gen)]
    b = torch.randint(-50, 50, (n,), generator=gen)

    def chain(a, b):
        perm = torch.arange(n, device=a.device)
        for key, asc in ((b, False), (a, True)):
            perm = perm[ops.sort_indices(key[perm], ascending=asc)]
        return perm

    exp = chain(a, b)
    got = chain(a.to(dev), b.to(dev))
    assert torch.equal(got.cpu(), exp)
    # and the host chain is the lexicographic order it stands for
    order = sorted(range(n), key=lambda i: (a[i].item() + 0.0, -b[i].item()))
    assert [(a[i].item(), b[i].item()) for i in exp.tolist()] == \
        [(a[i].item(), b[i].item()) for i in order]


# ------------------------------------------------------------- hash GROUP BY
def _check_groups(nat, dev, keys):
    gid, uniq = nat.hash_group_i64(keys.to(dev))
    gid, uniq = gid.cpu().long(), uniq.cpu()
    exp_uniq = torch.unique(keys)
    assert int(gid.min()) >= 0          # before anything indexes with gid
    g = exp_uniq.shape[0]
    assert uniq.shape[0] == g
    assert int(gid.max()) == g - 1
    assert torch.equal(torch.unique(gid), torch.arange(g))  # dense
    assert torch.equal(torch.sort(uniq).values, exp_uniq)  # no duplicate
    assert torch.equal(uniq[gid], keys)
    return gid, uniq


@pytest.mark.parametrize("n", [1, 4, 255, 257, 4097])
def test_hash_group_limit_keys(nat, dev, n):
    _check_groups(nat, dev, R.limit_keys_mixture(n, seed=n))


@pytest.mark.parametrize("n", [1, 2, 300])
def test_hash_group_int64_min_alone(nat, dev, n):
    gid, uniq = _check_groups(
        nat, dev, torch.full((n,), R.I64_MIN, dtype=torch.int64))
    assert uniq.tolist() == [R.I64_MIN] and gid.tolist() == [0] * n


@pytest.mark.parametrize("n", [1, 64, 255, 257, 4097])
def test_hash_group_all_distinct(nat, dev, n):
    """n distinct keys: load factor 1/2, the fullest the table gets."""
    gen = torch.Generator().manual_seed(20 + n)
    keys = torch.randperm(8 * n, generator=gen)[:n] - 4 * n
    keys = keys * 0x1E3779B97F4A7C15  # odd multiplier: distinct, all bits
    assert torch.unique(keys).shape[0] == n
    _check_groups(nat, dev, keys)


@pytest.mark.parametrize("n", [8, 32, 257, 4097])
def test_hash_group_cluster_wraps_table_end(nat, dev, n):
    """Up to 32 keys homed on the last two slots: probing must wrap to 0."""
    build, _, _ = R.wrap_cluster(n)
    mask = R.table_size(n) - 1
    homes = R.mix64(build.numpy()) & mask
    assert int((homes >= mask - 1).sum()) == min(n, 32)
    _check_groups(nat, dev, build)


def test_hash_agg_capture_limit_keys(nat, dev):
    """The capture form shares the kernels: the same INT64_MIN mixture on
    padded inputs, with sum / min / max columns."""
    n_cap, nrow = 4096, 3000
    gen = torch.Generator().manual_seed(31)
    keys = R.limit_keys_mixture(n_cap, seed=31)
    keys[nrow:] = torch.randint(1000, 1100, (n_cap - nrow,), generator=gen)
    f0 = R.spread_values(n_cap, gen)
    f1 = torch.randn(n_cap, generator=gen) * 5
    nrow_t = torch.tensor([nrow], device=dev, dtype=torch.int32)
    gcount = torch.full((1,), -1, device=dev, dtype=torch.int32)
    uniq, cnt, red = nat.hash_agg_capture(
        keys.to(dev), nrow_t, [f0.to(dev), f1.to(dev), f1.to(dev)],
        [0, 1, 2], 256, 128, gcount)
    uniq_ref, inv = torch.unique(keys[:nrow], return_inverse=True)
    g = uniq_ref.numel()
    assert R.I64_MIN in uniq_ref.tolist() and g <= 128
    assert int(gcount.item()) == g
    s, mn, mx, rows, a = R.segment_ref(f0[:nrow], inv, g)
    _, mn1, mx1, _, _ = R.segment_ref(f1[:nrow], inv, g)
    uniq, cnt = uniq.cpu(), cnt.cpu()
    order = torch.argsort(uniq[:g])
    assert torch.equal(uniq[:g][order], uniq_ref)
    assert torch.equal(cnt[:g][order], rows)
    err = (red[0].cpu()[:g][order].double() - s).abs()
    assert bool((err <= R.sum_bound(rows, a)).all())
    assert torch.equal(red[1].cpu()[:g][order], mn1.float())
    assert torch.equal(red[2].cpu()[:g][order], mx1.float())


# ----------------------------------------------------------------- hash join
def _check_join(nat, dev, lk, rk):
    l_idx, r_idx = nat.join_inner_i64(lk.to(dev), rk.to(dev))
    exp = R.join_pairs(lk, rk)
    assert l_idx.shape[0] == exp.shape[0]
    l_host = l_idx.cpu().long()
    assert bool((l_host[1:] >= l_host[:-1]).all())  # left-ordered output
    assert torch.equal(R.sorted_pairs(l_idx, r_idx), exp)
    return exp.shape[0]


@pytest.mark.parametrize("nl,nr", [(1, 1), (1, 257), (255, 1), (257, 255),
                                   (4097, 257), (257, 4097), (4097, 4097)])
def test_join_limit_keys_both_sides(nat, dev, nl, nr):
    lk = R.limit_keys_mixture(nl, seed=40 + nl)
    rk = R.limit_keys_mixture(nr, seed=41 + nr)
    if nl * nr > 1_000_000:  # keep the exact pair set small: thin the left
        lk = torch.where(torch.arange(nl) % 16 == 0, lk, lk * 0 + 10_000)
    total = _check_join(nat, dev, lk, rk)
    assert total > 0


def test_join_int64_min_only(nat, dev):
    lk = torch.tensor([R.I64_MIN, 5, R.I64_MIN, R.I64_MAX])
    rk = torch.tensor([7, R.I64_MIN, R.I64_MIN, R.I64_MIN + 1])
    assert _check_join(nat, dev, lk, rk) == 4
    assert _check_join(nat, dev, lk, torch.tensor([1, 2, 3])) == 0


def test_join_hot_key(nat, dev):
    lk = torch.full((300,), 42, dtype=torch.int64)
    assert _check_join(nat, dev, lk, lk.clone()) == 300 * 300


def test_join_disjoint_and_single_right_row(nat, dev):
    gen = torch.Generator().manual_seed(43)
    lk = torch.randint(0, 500, (4097,), generator=gen)
    assert _check_join(nat, dev, lk, lk[:257] + 1000) == 0
    assert _check_join(nat, dev, lk, lk[17:18].clone()) >= 1
    assert _check_join(nat, dev, lk, torch.tensor([-1])) == 0


@pytest.mark.parametrize("n", [8, 32, 257, 4097])
def test_join_cluster_wraps_table_end(nat, dev, n):
    """Build keys whose cluster wraps the table end; probes that hit, that
    miss inside the cluster and that miss past its end."""
    build, miss_inside, miss_past = R.wrap_cluster(n)
    gen = torch.Generator().manual_seed(n)
    lk = torch.cat([build, miss_inside, miss_past, build[:8]])
    lk = lk[torch.randperm(lk.shape[0], generator=gen)]
    assert _check_join(nat, dev, lk, build) == n + min(n, 8)
    assert _check_join(nat, dev, torch.cat([miss_inside, miss_past]),
                       build) == 0


@pytest.mark.parametrize("nl,nr", [(1, 1), (255, 257), (4097, 255)])
def test_join_left_exact(dev, nl, nr):
    from arkflow_amd import ops
    lk = R.limit_keys_mixture(nl, seed=50 + nl)
    rk = R.limit_keys_mixture(nr, seed=51 + nr)
    rk = rk[rk != -1] if nr > 1 else rk + 3   # some left rows stay unmatched
    lk = torch.where(torch.arange(nl) % 8 == 0, lk, lk * 0 - 1) \
        if nl > 1 else lk
    l_idx, r_idx = ops.join_left(lk.to(dev), rk.to(dev))
    exp = R.left_join_pairs(lk, rk)
    assert bool((exp[:, 1] == -1).any())
    l_host = l_idx.cpu().long()
    assert bool((l_host[1:] >= l_host[:-1]).all())
    assert torch.equal(R.sorted_pairs(l_idx, r_idx), exp)


def test_join_inner_refuses_float_keys_on_device(dev):
    from arkflow_amd import ops
    f = torch.tensor([1.5, 2.25], device=dev)
    i = torch.tensor([1, 2], device=dev)
    for lk, rk in ((f, f), (i, f), (f.double(), i)):
        with pytest.raises(TypeError):
            ops.join_inner(lk, rk)


# ------------------------------------------------------------ segment reduce
def _check_segment(nat, dev, vals, gids, g):
    s, mn, mx, rows, a = R.segment_ref(vals, gids, g)
    bound = R.sum_bound(rows, a)
    # the bound admits the plainest f32 summation of these very inputs
    assert bool(((R.f32_index_order_sum(vals, gids, g) - s).abs()
                 <= bound).all())
    dv, dg = vals.to(dev), gids.to(dev)
    got = nat.segment_reduce_f32(dv, dg, g, 0).cpu().double()
    err = (got - s).abs()
    bad = torch.nonzero(err > bound).flatten()
    assert bad.numel() == 0, \
        f"sum off in groups {bad[:5].tolist()}: err {err[bad[:5]].tolist()}" \
        f" bound {bound[bad[:5]].tolist()}"
    assert torch.equal(nat.segment_reduce_f32(dv, dg, g, 1).cpu(), mn.float())
    assert torch.equal(nat.segment_reduce_f32(dv, dg, g, 2).cpu(), mx.float())


@pytest.fixture(scope="module")
def seg_inputs():
    gen = torch.Generator().manual_seed(60)
    n = 20_000
    return R.spread_values(n, gen), torch.randint(
        0, 1 << 30, (n,), generator=gen)


@pytest.mark.parametrize("g", [1, 2, 777, 2047, 2048, 2049, 5000])
@pytest.mark.parametrize("n", [1, 255, 257, 20_000])
def test_segment_reduce_exact(nat, dev, seg_inputs, n, g):
    vals, raw = seg_inputs
    gids = (raw[:n] % g).to(torch.int32)
    _check_segment(nat, dev, vals[:n], gids, g)


@pytest.mark.parametrize("g", [40, 2048, 2049, 6000])
def test_segment_reduce_empty_groups(nat, dev, seg_inputs, g):
    """g larger than the largest gid used: the groups past it, and the holes
    between, give 0, +inf and -inf."""
    vals, raw = seg_inputs
    n = 257
    gids = (raw[:n] % 30 * (g // 40)).to(torch.int32)
    assert int(gids.max()) < g - 1
    _check_segment(nat, dev, vals[:n], gids, g)
    dv, dg = vals[:n].to(dev), gids.to(dev)
    last = [nat.segment_reduce_f32(dv, dg, g, op)[-1].item()
            for op in (0, 1, 2)]
    assert last == [0.0, float("inf"), float("-inf")]


@pytest.mark.parametrize("g", [1, 2049])
def test_segment_reduce_all_rows_one_group(nat, dev, seg_inputs, g):
    vals, _ = seg_inputs
    gids = torch.full((20_000,), g - 1, dtype=torch.int32)
    _check_segment(nat, dev, vals, gids, g)


def test_segment_reduce_no_rows_no_groups(nat, dev):
    for op in (0, 1, 2):
        out = nat.segment_reduce_f32(
            torch.empty(0, device=dev),
            torch.empty(0, device=dev, dtype=torch.int32), 0, op)
        assert out.shape == (0,) and out.dtype == torch.float32


@pytest.mark.parametrize("g", [8, 2049])
def test_segment_min_max_propagate_nan(nat, dev, seg_inputs, g):
    """A NaN of either sign makes its group's min and max NaN; every other
    group is unaffected."""
    vals, raw = seg_inputs
    n = 4097
    vals = vals[:n].clone()
    gids = (raw[:n] % g).to(torch.int32)
    nan_pos = torch.tensor([0x7fc00000], dtype=torch.int32).view(torch.float32)
    nan_neg = torch.tensor([-0x400000], dtype=torch.int32).view(torch.float32)
    assert nan_neg.view(torch.int32).item() < 0 and bool(nan_neg.isnan())
    i_pos, i_neg = 1000, 3000  # rows of groups 2 and 5, among other rows
    gids[i_pos], gids[i_neg] = 2, 5
    vals[i_pos], vals[i_neg] = nan_pos[0], nan_neg[0]
    assert vals[i_pos].view(torch.int32).item() > 0
    assert vals[i_neg].view(torch.int32).item() < 0
    _, mn, mx, _, _ = R.segment_ref(vals, gids, g)
    assert int(mn.isnan().sum()) == 2 and int(mx.isnan().sum()) == 2
    for op, ref in ((1, mn), (2, mx)):
        got = nat.segment_reduce_f32(vals.to(dev), gids.to(dev), g, op).cpu()
        assert torch.equal(got.isnan(), ref.isnan())
        keep = ~ref.isnan()
        assert torch.equal(got[keep], ref.float()[keep])


def test_segment_count_exact_past_2_pow_24(dev):
    """2^24 + 3 rows in one group: the smallest count an f32 sum of ones
    gets wrong."""
    from arkflow_amd import ops
    n = (1 << 24) + 3
    ones = torch.ones(n, device=dev)
    gid = torch.zeros(n, device=dev, dtype=torch.int32)
    got = ops.segment_reduce(ones, gid, 1, "count")
    assert got.dtype == torch.int64 and got.tolist() == [n]
