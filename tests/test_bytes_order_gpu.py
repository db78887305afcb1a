"""ops.bytes_rank / ops.bytes_compare on the device against the plain Python
reference: bytes order is bytewise, unsigned, a proper prefix first. Every
comparison is exact. The cases sit where the kernels can go wrong: the 7-byte
chunk boundaries of the rank, NUL and high bytes, long common prefixes (many
rounds), many ties per round, the 1024-row scan tiles and 4096-row sort tiles,
and columns whose bytes do not start at an aligned address."""
import random

import pytest
import torch

from arkflow_amd import ops
from arkflow_amd.batch import Column

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    ops.require_native()
    return torch.device("cuda:0")


def _chunk_boundaries():
    rows = []
    for ln in range(25):
        p = bytes((7 * ln + i) % 251 + 1 for i in range(ln))
        # differ right after a common prefix of ln bytes; proper prefixes
        rows += [p + b"a", p + b"b", p + b"a\x00", p, p + b"\x00", p + b"ab"]
    rows += [b"x" * 7, b"x" * 14, b"x" * 21, b"x" * 7, b"x" * 8, b"x" * 6,
             b"x" * 13, b"x" * 15, b"x" * 20, b"x" * 22, b"x" * 14]
    random.Random(1).shuffle(rows)
    return rows


def _random_rows(seed, n, alphabet, max_len):
    rng = random.Random(seed)
    return [bytes(rng.choice(alphabet) for _ in range(rng.randint(0, max_len)))
            for _ in range(n)]


def _low_card(seed, n):
    """12-byte values, 6 of them distinct, that share their first 7 bytes:
    the first round leaves one open segment that spans every tile."""
    rng = random.Random(seed)
    vals = [b"device-" + s for s in (b"00001", b"00002", b"0000\xff",
                                     b"1\x000\x000", b"zzzzz", b"00000")]
    return [rng.choice(vals) for _ in range(n)]


def _nul_rows():
    rows = [b"ab", b"ab\x00", b"ab\x00\x00", b"ab\x00c"] * 5 + [b"a", b""]
    random.Random(2).shuffle(rows)
    return rows


def _unsigned_rows():
    edge = [b"\x00", b"\x7f", b"\x80", b"\xff"]
    rows = [a + b"mid" + b for a in edge for b in edge] + edge \
        + [b"mid" + b for b in edge] + [a + b"mid" for a in edge]
    random.Random(3).shuffle(rows)
    return rows


LONG = bytes(range(256)) + bytes(44)  # 300 bytes
CASES = {
    "one_row": [b"solo"],
    "all_equal": [b"same-value"] * 70,
    "all_empty": [b""] * 33,
    "empty_mixed": [b"", b"a", b"", b"\x00", b"b", b"", b"a"],
    "prefix_nul": _nul_rows(),
    "unsigned": _unsigned_rows(),
    "chunk_boundaries": _chunk_boundaries(),
    "long_prefix": [LONG[:-1] + b"\x02", LONG[:-1] + b"\x01", LONG, LONG,
                    LONG[:-1], LONG[:-1] + b"\x01"],
    "two_letters_5000": _random_rows(4, 5000, b"ab", 20),
    "all_bytes": _random_rows(5, 3000, bytes(range(256)), 40),
    "rows_1023": _low_card(6, 1023),
    "rows_1025": _low_card(7, 1025),
    "rows_4097": _low_card(8, 4097),
}
_REF = {}


def _ref_rank(name):
    """Reference rank of a case, computed once and shared."""
    if name not in _REF:
        rows = CASES[name]
        order = {v: i for i, v in enumerate(sorted(set(rows)))}
        _REF[name] = [order[v] for v in rows]
    return _REF[name]


def _cmp(a, b):
    return (a > b) - (a < b)


def test_empty_column(dev):
    col = Column.from_bytes([]).to(dev)
    r = ops.bytes_rank(col)
    assert r.dtype == torch.int64 and r.shape == (0,) and r.is_cuda
    c = ops.bytes_compare(col, b"x")
    assert c.dtype == torch.int8 and c.shape == (0,)
    assert ops.bytes_compare(col, col).shape == (0,)


@pytest.mark.parametrize("name", list(CASES))
def test_rank(dev, name):
    rows = CASES[name]
    r = ops.bytes_rank(Column.from_bytes(rows).to(dev))
    assert r.dtype == torch.int64 and r.is_cuda
    assert r.cpu().tolist() == _ref_rank(name)


def test_rank_matches_cpu_reference(dev):
    rows = CASES["chunk_boundaries"]
    cpu = ops.bytes_rank(Column.from_bytes(rows))
    assert cpu.tolist() == _ref_rank("chunk_boundaries")


def test_rank_of_slice_and_take(dev):
    rows = CASES["all_bytes"]
    big = Column.from_bytes(rows).to(dev)
    # Column.slice: the bytes start in the middle of the buffer, at any
    # alignment
    for start, length in ((5, 1500), (1001, 1024)):
        part = rows[start:start + length]
        order = {v: i for i, v in enumerate(sorted(set(part)))}
        got = ops.bytes_rank(big.slice(start, length))
        assert got.cpu().tolist() == [order[v] for v in part]
        # offsets that keep their base: offsets[0] != 0
        raw = Column("binary", big.data,
                     big.offsets[start:start + length + 1])
        assert int(raw.offsets[0]) != 0
        assert ops.bytes_rank(raw).cpu().tolist() == [order[v] for v in part]
        lit = part[7]
        assert ops.bytes_compare(raw, lit).cpu().tolist() == \
            [_cmp(v, lit) for v in part]
    idx = torch.tensor(random.Random(9).sample(range(len(rows)), 700),
                       device=dev)
    part = [rows[i] for i in idx.cpu().tolist()]
    order = {v: i for i, v in enumerate(sorted(set(part)))}
    assert ops.bytes_rank(big.take(idx)).cpu().tolist() == \
        [order[v] for v in part]


@pytest.mark.parametrize("name", list(CASES))
def test_compare_columns(dev, name):
    """Against a rotated copy of itself: -1 / 0 / +1 per row."""
    rows = CASES[name]
    k = max(1, len(rows) // 3) % len(rows)
    rot = rows[k:] + rows[:k]
    a = Column.from_bytes(rows).to(dev)
    b = Column.from_bytes(rot).to(dev)
    got = ops.bytes_compare(a, b)
    assert got.dtype == torch.int8
    assert got.cpu().tolist() == [_cmp(x, y) for x, y in zip(rows, rot)]
    assert ops.bytes_compare(a, a).cpu().tolist() == [0] * len(rows)


@pytest.mark.parametrize("name", list(CASES))
def test_compare_literal(dev, name):
    rows = CASES[name]
    col = Column.from_bytes(rows).to(dev)
    longest = max(rows, key=len)
    lits = [b"", rows[len(rows) // 2], longest + b"\x00tail",
            longest[:max(len(longest) - 1, 0)], longest[:3], b"ab", b"\x80"]
    for lit in lits:
        got = ops.bytes_compare(col, lit).cpu().tolist()
        assert got == [_cmp(v, lit) for v in rows], lit


def test_compare_checks_its_arguments(dev):
    a = Column.from_bytes([b"a", b"b"]).to(dev)
    with pytest.raises(ValueError):
        ops.bytes_compare(a, Column.from_bytes([b"a"]).to(dev))
    with pytest.raises(TypeError):
        ops.bytes_rank(Column.from_numeric([1, 2]).to(dev))
