"""Per-stripe erasure patterns, host side: the multi-table entry points are
exported, and build_pattern_tables produces — per distinct (erased, want)
pair — exactly the tables the oracle builds for that pattern.  No GPU.
"""
import ctypes
import os

import numpy as np
import pytest

import oracle
from lizardfs_amd import lib as L
from lizardfs_amd.ec import build_pattern_tables

PART_LEN = 64


def test_multi_symbols_exported():
    so = ctypes.CDLL(os.path.join(os.path.dirname(L.__file__), "liblizec.so"))
    for name in ("lizec_ec_encode_batch_multi", "lizec_ec_plan_create_multi"):
        assert hasattr(so, name), f"liblizec.so does not export {name}"


def _mask(idx):
    v = 0
    for i in idx:
        v |= 1 << int(i)
    return v


def _random_patterns(k, m, S, seed):
    """Seeded pattern list with repeats and want sizes from 1 to m."""
    rng = np.random.default_rng(seed)
    pool = [tuple(sorted(rng.choice(k + m, m, replace=False).tolist()))
            for _ in range(max(2, S // 3))]
    erased, want = [], []
    for s in range(S):
        e = pool[int(rng.integers(len(pool)))]
        n = int(rng.integers(1, m + 1)) if s else m   # stripe 0 wants all m
        w = tuple(sorted(rng.choice(e, n, replace=False).tolist()))
        erased.append(set(e))
        want.append(set(w))
    erased[-1], want[-1] = set(erased[0]), set(want[0])   # a sure repeat
    return erased, want


def _host_encode(tbl, srcs, ndests, size):
    """liblizec's host ec_encode_data (the drop-in CPU entry point)."""
    lib = L.lib()
    dests = [np.zeros(size, np.uint8) for _ in range(ndests)]
    sp = (ctypes.c_void_p * len(srcs))(*[a.ctypes.data for a in srcs])
    dp = (ctypes.c_void_p * ndests)(*[a.ctypes.data for a in dests])
    tbl = np.ascontiguousarray(tbl)
    lib.ec_encode_data(size, len(srcs), ndests,
                       tbl.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                       sp, dp)
    return dests


@pytest.mark.parametrize("k,m,S", [(8, 2, 24), (3, 1, 9), (32, 6, 12)])
def test_build_pattern_tables(k, m, S):
    erased, want = _random_patterns(k, m, S, seed=1000 * k + m)
    tables, index, slots = build_pattern_tables(k, m, erased, want)

    oc = max(len(w) for w in want)
    pairs = {(_mask(e), _mask(w)) for e, w in zip(erased, want)}
    assert tables.dtype == np.uint8 and tables.shape == (len(pairs), 32 * k * oc)
    assert index.dtype == np.uint32 and index.shape == (S,)
    assert slots.shape == (S, oc)
    assert len(pairs) < S, "the pattern list must contain repeats"
    assert len({len(w) for w in want}) > 1 or m == 1, "mixed want sizes"

    rng = np.random.default_rng(7)
    data = [rng.integers(0, 256, PART_LEN, np.uint8) for _ in range(k)]
    parts = data + oracle.rs_encode(k, m, data, PART_LEN)
    all_parts = (1 << (k + m)) - 1
    for s in range(S):
        present = all_parts & ~_mask(erased[s])
        exp, ic, noc = oracle.rs_make_tables(k, m, present, present,
                                             _mask(want[s]))
        assert (ic, noc) == (k, len(want[s]))
        row = tables[index[s]]
        assert np.array_equal(row[:32 * k * noc], exp), f"stripe {s}"
        assert not row[32 * k * noc:].any(), f"stripe {s}: unused rows"
        assert slots[s].tolist() == sorted(want[s]) + [-1] * (oc - noc)

        srcs = [parts[i] for i in range(k + m) if i not in erased[s]]
        got = _host_encode(row, srcs, oc, PART_LEN)
        for j, part in enumerate(slots[s]):
            if part >= 0:
                assert np.array_equal(got[j], parts[part]), \
                    f"stripe {s}: slot {j} (part {part})"
            else:
                assert not got[j].any(), f"stripe {s}: unused slot {j}"


def test_want_defaults_to_erased_and_array_input():
    erased = np.array([[0, 9], [3, 4], [9, 0], [8, 9]])
    tables, index, slots = build_pattern_tables(8, 2, erased)
    assert tables.shape == (3, 32 * 8 * 2)
    assert index[0] == index[2] and len(set(index.tolist())) == 3
    assert slots.tolist() == [[0, 9], [3, 4], [0, 9], [8, 9]]
    t2, i2, s2 = build_pattern_tables(8, 2, [set(r) for r in erased.tolist()])
    assert np.array_equal(tables, t2) and np.array_equal(index, i2)
    assert np.array_equal(slots, s2)


@pytest.mark.parametrize("erased", [
    [{0, 1}, {2}],            # too few
    [{0, 1}, {2, 3, 4}],      # too many
    [{0, 1}, {5, 5}],         # a repeated index is one part
])
def test_erased_size_must_be_m(erased):
    with pytest.raises(ValueError):
        build_pattern_tables(8, 2, erased)


@pytest.mark.parametrize("want", [
    [{0}, {4}],               # 4 is not erased in stripe 1
    [{0, 1}, {2, 3, 9}],      # superset
    [{0}, set()],             # empty
])
def test_want_must_be_nonempty_subset(want):
    with pytest.raises(ValueError):
        build_pattern_tables(8, 2, [{0, 1}, {2, 3}], want)
