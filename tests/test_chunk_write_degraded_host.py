"""lizec_degraded_write_table, lizec_chunk_write_degraded_host and
chunkwrite.write_chunks_degraded_host / plan_write_degraded on the CPU,
bit-exact against the reference's route through the oracle
(chunk_write_degraded_cases.py).  No GPU is needed.

  cells      [slice-layout], the eight writes of the helper in one call per
             availability pattern: healthy; one data part lost that is FILL
             in the first touched row; one that is FILL in the last row
             only; one that is NEW wherever the write touches it (with a
             second parity, one parity lost as well); m data parts at once;
             one data part and one parity part.  A write without a column
             of the kind stays healthy in that call.  The slot of a lost
             part points at random bytes.
  mask       slots outside a write's masks point at random bytes, or carry
             address 0 and count 0: the same output; a mask that leaves out
             a slot whose table column is not zero: the column counts as zeros
  builder    the composite table applied with oracle.ec_encode_data equals
             rebuild-then-encode, for every run of new columns and every
             single and double loss; healthy rows; the xor read-modify-write
             form; refusals
  refusals   every LIZEC_EINVAL of lizec.h, the arena left as it was
  python     plan_write_degraded, write_chunks_degraded_host
"""
import ctypes
import itertools

import numpy as np
import pytest

import chunk_write_cases as C
import chunk_write_degraded_cases as D
import oracle

LIZEC_OK, LIZEC_EINVAL = D.LIZEC_OK, D.LIZEC_EINVAL
BLOCK = C.BLOCK

CELLS = [(s, l) for s in D.SLICES for l in ("il", "odd")] + \
    [("ec32", "fast"), ("ec32", "data4"), ("xor3", "fast")]


def make_case(name, layout, seed=1):
    sl, lay = D.SLICES[name], D.LAYOUTS[layout]
    return D.Case(sl, lay, D.the_writes(sl.ks, layout == "fast"), seed)


def test_the_symbols_exist():
    from lizardfs_amd import lib as L
    lib = L.lib()
    assert lib.lizec_degraded_write_table
    assert lib.lizec_chunk_write_degraded_host
    assert lib.lizec_chunk_write_degraded_batch
    assert lib.lizec_impl_chunk_write_degraded_check


@pytest.mark.parametrize("name,layout", CELLS,
                         ids=[f"{s}-{l}" for s, l in CELLS])
def test_cell(name, layout):
    case = make_case(name, layout)
    for pattern in D.PATTERNS:
        if not case.set_pattern(pattern) and pattern != "healthy":
            continue
        rc, arena = case.run_host()
        assert rc == LIZEC_OK
        case.check(arena)


@pytest.mark.parametrize("name", ["xor3", "ec32", "ec29", "ec87-rows5"])
def test_the_mask_is_obeyed(name):
    case = make_case(name, "odd", seed=3)
    for pattern in ("healthy", "fill-first", "m-data"):
        case.set_pattern(pattern)
        for spare in ("swap", "zero", "null"):
            rc, arena = case.run_host(spare)
            assert rc == LIZEC_OK
            case.check(arena)


@pytest.mark.parametrize("name", ["xor3", "ec32", "ec87-rows5"])
def test_a_slot_with_a_coefficient_outside_the_mask_is_not_read(name):
    """The builder's masks leave out only slots whose column is zero, which
    no output can tell from a slot that was read.  Here every mask loses a
    fill slot whose column is not zero: that column counts as zeros."""
    case = make_case(name, "odd", seed=9)
    case.set_pattern("healthy")
    before = case.want.copy()
    assert case.drop_a_mask_bit() >= 2
    assert not np.array_equal(before, case.want)
    rc, arena = case.run_host()
    assert rc == LIZEC_OK
    case.check(arena)


@pytest.mark.parametrize("name", ["xor3", "ec52", "ec29"])
def test_a_healthy_call_equals_the_healthy_entry(name):
    from lizardfs_amd import lib as L
    case = make_case(name, "odd", seed=5)
    case.set_pattern("healthy")
    rc, arena = case.run_host()
    assert rc == LIZEC_OK
    other = np.full(case.size, C.FILL, np.uint8)
    wr, fp, fn, pp = case.writes.arrays(case.store.host.ctypes.data,
                                        case.data.ctypes.data,
                                        other.ctypes.data)
    rc = L.lib().lizec_chunk_write_host(
        case.sl.m, C.encode_table(case.sl).ctypes.data_as(D.u8p),
        ctypes.c_void_p(wr.ctypes.data), len(wr), fp.ctypes.data_as(D.u64p),
        fn.ctypes.data_as(D.u32p), case.sl.ks, case.lay.stride,
        pp.ctypes.data_as(D.u64p))
    assert rc == LIZEC_OK
    assert np.array_equal(arena, other)


# --------------------------------------------------------------------------
# the table builder

BUILDER_SLICES = ["xor3", "ec21", "ec32", "ec52", "ec29", "ec87-rows7"]


def runs(ks):
    """The new-column masks a write can produce in a row: runs of bits."""
    return [((1 << hi) - 1) & ~((1 << lo) - 1)
            for lo in range(ks) for hi in range(lo + 1, ks + 1)]


@pytest.mark.parametrize("name", BUILDER_SLICES)
def test_composite_table_equals_rebuild_then_encode(name):
    sl = D.SLICES[name]
    ks, m, n = sl.ks, sl.m, sl.ks + sl.m
    size = 64
    rng = np.random.default_rng(7)
    old_data = [rng.integers(0, 256, size, np.uint8) for _ in range(ks)]
    old = old_data + C.parity_of(sl, old_data, size)
    new = [rng.integers(0, 256, size, np.uint8) for _ in range(ks)]
    junk = rng.integers(0, 256, size, np.uint8)
    zeros = np.zeros(size, np.uint8)
    # with one parity a double loss is refused where a fill column is lost
    losses = [(p,) for p in range(n)] + \
        list(itertools.combinations(range(n), 2))
    built = refused = 0
    for new_mask in runs(ks):
        for lost in losses:
            avail = [p for p in range(n) if p not in lost]
            lost_fill = [c for c in lost if c < ks and not (new_mask >> c) & 1]
            rc, tbl, mask = D.build_table(
                sl, new_mask, (1 << ks) - 1, sum(1 << p for p in avail),
                range(n))
            if lost_fill and len(avail) < ks:
                assert rc == LIZEC_EINVAL
                refused += 1
                continue
            assert rc == LIZEC_OK, (new_mask, lost)
            built += 1
            cols = [new[c] if (new_mask >> c) & 1 else
                    D.rebuild(sl, avail, c, old, size) if c in lost_fill else
                    old[c] for c in range(ks)]
            want = C.parity_of(sl, cols, size)
            # an unavailable part is read as junk, a slot outside the mask
            # as well: their columns are zero
            assert not any((mask >> p) & 1 for p in lost)
            srcs = [new[c] if (new_mask >> c) & 1 else zeros
                    for c in range(ks)] + \
                [old[p] if (mask >> p) & 1 else junk for p in range(n)]
            got = [np.zeros(size, np.uint8) for _ in range(m)]
            oracle.ec_encode_data(np.ascontiguousarray(tbl),
                                  [np.ascontiguousarray(a) for a in srcs],
                                  got)
            for r in range(m):
                assert np.array_equal(got[r], want[r]), (new_mask, lost, r)
            if not lost_fill:
                fill = ((1 << ks) - 1) & ~new_mask
                assert mask == fill
    assert built
    assert bool(refused) == (m == 1)


@pytest.mark.parametrize("name", BUILDER_SLICES)
def test_a_healthy_row_has_the_encode_table(name):
    sl = D.SLICES[name]
    ks, n = sl.ks, sl.ks + sl.m
    enc = C.encode_table(sl).reshape(sl.m, ks, 32)
    for new_mask in runs(ks):
        for have in ((1 << ks) - 1, new_mask | 1):
            rc, tbl, mask = D.build_table(sl, new_mask, have, (1 << n) - 1,
                                          range(n))
            assert rc == LIZEC_OK
            tbl = tbl.reshape(sl.m, ks + n, 32)
            fill = have & ~new_mask
            assert mask == fill
            for c in range(ks):
                if (new_mask >> c) & 1:
                    assert np.array_equal(tbl[:, c], enc[:, c])
                    assert not tbl[:, ks + c].any()
                else:
                    assert not tbl[:, c].any()
                    if (fill >> c) & 1:
                        assert np.array_equal(tbl[:, ks + c], enc[:, c])
                    else:
                        assert not tbl[:, ks + c].any()
            assert not tbl[:, 2 * ks:].any()


def test_xor_read_modify_write():
    """xor3, column 0 overwritten, column 2 lost: new ^ old ^ old parity; the
    readable fill column 1 cancels and is not read."""
    sl = D.SLICES["xor3"]
    rc, tbl, mask = D.build_table(sl, 0b001, 0b111, 0b1011, range(4))
    assert rc == LIZEC_OK
    assert mask == 0b1001     # the overwritten column and the parity
    ones = oracle.init_tables(np.ones(1, np.uint8))
    tbl = tbl.reshape(1, 3 + 4, 32)
    for col in range(7):
        if col in (0, 3, 6):
            assert np.array_equal(tbl[0, col], ones)
        else:
            assert not tbl[0, col].any()
    # slots in another order, and fewer of them
    rc, tbl, mask = D.build_table(sl, 0b001, 0b111, 0b1011, [3, 1, 0])
    assert rc == LIZEC_OK and mask == 0b101


def test_a_survivor_without_the_row_needs_no_slot():
    """ec(3,2), column 0 lost and a fill, column 1 overwritten, column 2
    past its part's end: part 2 is among the first k available parts but
    counts as zeros, so the table needs no slot for it and no column of it;
    the rebuild takes the old bytes of part 1 and parity 0."""
    sl = D.SLICES["ec32"]
    rc, full, fmask = D.build_table(sl, 0b010, 0b011, 0b11110, range(5))
    assert rc == LIZEC_OK and fmask == 0b01010
    rc, tbl, mask = D.build_table(sl, 0b010, 0b011, 0b11110, [3, 1])
    assert rc == LIZEC_OK and mask == 0b11
    full = full.reshape(2, 3 + 5, 32)
    tbl = tbl.reshape(2, 3 + 2, 32)
    assert np.array_equal(tbl[:, :3], full[:, :3])
    assert np.array_equal(tbl[:, 3], full[:, 3 + 3]) and tbl[:, 3].any()
    assert np.array_equal(tbl[:, 4], full[:, 3 + 1]) and tbl[:, 4].any()
    assert not full[:, 3 + 2].any()
    # the old column 1 without the row as well: parity 0 alone
    rc, tbl, mask = D.build_table(sl, 0b010, 0b001, 0b11110, [3])
    assert rc == LIZEC_OK and mask == 0b1
    # with the row, part 2 is needed
    assert D.build_table(sl, 0b010, 0b111, 0b11110, [3, 1])[0] == LIZEC_EINVAL
    # xor3: column 2 past its end, column 1 lost: parity and column 0 do
    x = D.SLICES["xor3"]
    rc, tbl, mask = D.build_table(x, 0b001, 0b011, 0b1101, [3, 0])
    assert rc == LIZEC_OK and mask == 0b11


def test_builder_refusals():
    sl = D.SLICES["ec32"]
    full = 0b11111

    def rc(new=0b001, have=0b111, avail=full, slots=range(5), sl=sl):
        return D.build_table(sl, new, have, avail, list(slots))[0]

    assert rc() == LIZEC_OK
    assert rc(new=0b1000) == LIZEC_EINVAL        # a column outside the slice
    assert rc(have=0b1111) == LIZEC_EINVAL
    assert rc(avail=0b111111) == LIZEC_EINVAL
    assert rc(slots=[0, 1, 2, 3, 5]) == LIZEC_EINVAL   # no such part
    assert rc(slots=[0, 1, 2, 3, 3]) == LIZEC_EINVAL   # named twice
    assert rc(slots=[0, 2, 3, 4]) == LIZEC_EINVAL      # fill column 1: no slot
    assert rc(slots=[0, 2, 3, 4], new=0b011) == LIZEC_OK
    assert rc(slots=[]) == LIZEC_EINVAL
    assert rc(slots=list(range(5)) * 7) == LIZEC_EINVAL   # 35 slots
    # a lost fill column and fewer than k parts: "Not enough chunkservers"
    assert rc(avail=0b10001) == LIZEC_EINVAL
    assert rc(avail=0b10001, new=0b110) == LIZEC_OK    # nothing to rebuild
    assert rc(avail=0b11001) == LIZEC_OK
    # a survivor without a slot
    assert rc(avail=0b11001, slots=[0, 3]) == LIZEC_EINVAL
    # xor with two parities
    assert D.build_table(C.Slice("xor", 3), 1, 7, 15, range(4))[0] == LIZEC_OK
    from lizardfs_amd import lib as L
    tbl = np.zeros(32 * 7 * 2, np.uint8)
    mask = ctypes.c_uint32()
    slots = np.arange(4, dtype=np.uint8)
    fn = L.lib().lizec_degraded_write_table
    args = (1, 7, 15, slots.ctypes.data_as(D.u8p), 4,
            tbl.ctypes.data_as(D.u8p), ctypes.byref(mask))
    assert fn(3, 2, 1, *args) == LIZEC_EINVAL
    assert fn(0, 1, 0, *args) == LIZEC_EINVAL
    assert fn(33, 1, 0, *args) == LIZEC_EINVAL
    assert fn(3, 0, 0, *args) == LIZEC_EINVAL
    assert fn(3, 33, 0, *args) == LIZEC_EINVAL
    assert fn(3, 1, 0, 1, 7, 15, None, 4, tbl.ctypes.data_as(D.u8p),
              ctypes.byref(mask)) == LIZEC_EINVAL
    assert fn(3, 1, 0, 1, 7, 15, slots.ctypes.data_as(D.u8p), 4, None,
              ctypes.byref(mask)) == LIZEC_EINVAL
    assert fn(3, 1, 0, 1, 7, 15, slots.ctypes.data_as(D.u8p), 4,
              tbl.ctypes.data_as(D.u8p), None) == LIZEC_EINVAL


# --------------------------------------------------------------------------
# refusals of the call

def refusal_edits(case, good):
    """(edit, keyword overrides) of every refusal of lizec.h; `good` are the
    arrays (wr, op, on, pp) of a call that is accepted."""
    def field(i, name, value):
        def edit(a):
            a["wr"][name][i] = value
        return edit

    def item(name, at, value):
        def edit(a):
            a[name][at] = value
        return edit

    def null(name):
        def edit(a):
            a[name] = None
        return edit

    out = [(null(n), {}) for n in ("tbl", "masks", "index", "wr", "op", "on",
                                   "pp")]
    out += [(None, kw) for kw in (
        dict(num=0), dict(rows=0), dict(rows=33), dict(ks=0), dict(ks=33),
        dict(srcs=0), dict(srcs=33), dict(ntables=0), dict(stride=65535))]
    out += [(e, {}) for e in (
        field(0, "from", 65536), field(3, "to", 65537), field(3, "to", 13),
        field(1, "block_count", 0), field(1, "first_block", 1048576 - 5),
        field(2, "data", 0), field(1, "data_stride", 65535),
        field(1, "par_stride", 65535),
        field(0, "crcs", int(good[0]["crcs"][0]) + 1),
        item("on", (0, 1), 32769),
        item("index", (0, 0), len(case.masks)),
        item("index", (1, 1), len(case.masks)),
        item("index", (3, 2), 0xFFFFFFFF),
        item("masks", 0, 1 << case.nparts),
        item("masks", len(case.masks) - 1, 0x80000000),
        # a slot in a mask with a count and no address
        item("op", (0, int(case.masks[case.index[0, 0]]).bit_length() - 1),
             0),
        lambda a: (a["pp"].__setitem__((2, slice(None)), 0),
                   field(2, "crcs", 0)(a)))]
    return out


def call_edited(case, fn, head, tail, good, edit, kw):
    a = dict(tbl=case.tbl.copy(), masks=case.masks.copy(),
             index=case.index.copy(), wr=good[0].copy(), op=good[1].copy(),
             on=good[2].copy(), pp=good[3].copy())
    if edit:
        edit(a)

    def ptr(x, t):
        return None if x is None else x.ctypes.data_as(t)
    return fn(*head, kw.get("rows", case.sl.m), ptr(a["tbl"], D.u8p),
              kw.get("ntables", len(case.masks)), ptr(a["masks"], D.u32p),
              ptr(a["index"], D.u32p),
              None if a["wr"] is None else ctypes.c_void_p(
                  a["wr"].ctypes.data),
              kw.get("num", len(good[0])), ptr(a["op"], D.u64p),
              ptr(a["on"], D.u32p), kw.get("srcs", case.nparts),
              kw.get("ks", case.sl.ks), kw.get("stride", case.lay.stride),
              ptr(a["pp"], D.u64p), *tail)


def test_refusals_then_a_good_call():
    from lizardfs_amd import lib as L
    sl, lay = D.SLICES["ec32"], D.LAYOUTS["odd"]
    case = D.Case(sl, lay, D.the_writes(sl.ks, False)[:4], seed=17)
    case.set_pattern("fill-first")
    arena = np.full(case.size, C.FILL, np.uint8)
    good = case.arrays(case.store.host.ctypes.data, case.data.ctypes.data,
                       arena.ctypes.data)
    assert int(case.masks[case.index[0, 0]])
    fn = L.lib().lizec_chunk_write_degraded_host
    for edit, kw in refusal_edits(case, good):
        assert call_edited(case, fn, (), (), good, edit, kw) == LIZEC_EINVAL
    assert (arena == C.FILL).all()
    assert call_edited(case, fn, (), (), good, None, {}) == LIZEC_OK
    case.check(arena)


# --------------------------------------------------------------------------
# the Python layer

def slice_type(name):
    from lizardfs_amd import slice_traits as st
    sl = D.SLICES[name]
    return st.K_XOR2 + sl.ks - 2 if D.is_xor(sl) else \
        st.ec_slice_type(sl.ks, sl.m)


def test_plan_write_degraded():
    from lizardfs_amd import chunkwrite as W
    t = slice_type("ec32")
    N, F, A, X = W.NEW, W.FILL, W.ABSENT, W.LOST
    # 7 blocks; blocks 1..5: row 0 fills column 0, row 1 is whole
    healthy = W.plan_write(t, 7, 1, 5)
    plan = W.plan_write_degraded(t, range(5), 7, 1, 5)
    assert plan == healthy
    plan = W.plan_write_degraded(t, [1, 2, 3, 4], 7, 1, 5)
    assert plan.rows == [(0, [X, N, N]), (1, [N, N, N])]
    assert plan.read_parts == [1, 2, 3]
    assert plan.packets == [(1, 0), (1, 1), (2, 0), (2, 1),
                            (3, 0), (3, 1), (4, 0), (4, 1)]
    # a lost part that is NEW wherever it is touched: nothing to rebuild
    plan = W.plan_write_degraded(t, [0, 2, 3], 7, 1, 5)
    assert plan.rows == healthy.rows and plan.read_parts == [0]
    assert plan.packets == [(0, 1), (2, 0), (2, 1), (3, 0), (3, 1)]
    # fill in the last row only: 0..3 of 7 blocks, columns 1 and 2 of row 1
    plan = W.plan_write_degraded(t, [0, 1, 3, 4], 7, 0, 4)
    assert plan.rows == [(0, [N, N, N]), (1, [N, F, X])]
    assert plan.read_parts == [0, 1, 3]
    # two data parts lost, one parity: fewer than k parts
    assert W.plan_write_degraded(t, [2, 4], 7, 1, 5) is None
    assert W.plan_write_degraded(t, [2, 4], 7, 0, 6) is not None
    # past the chunk's end a lost column is ABSENT, not rebuilt
    plan = W.plan_write_degraded(t, [0, 1, 3, 4], 4, 6, 1)
    assert plan.rows == [(2, [N, A, A])] and plan.read_parts == []
    # a survivor that does not reach the row is not read: 4 blocks, block 4
    plan = W.plan_write_degraded(t, [1, 2, 3, 4], 4, 4, 1)
    assert plan.rows == [(1, [X, N, A])] and plan.read_parts == [3]
    # xor3: parity is part 0
    x = slice_type("xor3")
    plan = W.plan_write_degraded(x, [0, 1, 2], 7, 0, 1)
    assert plan.rows == [(0, [N, F, X])]
    assert plan.read_parts == [0, 1, 2]
    assert plan.packets == [(1, 0), (0, 0)]
    assert W.plan_write_degraded(x, [1, 2], 7, 0, 1) is None
    with pytest.raises(ValueError):
        W.plan_write_degraded(t, [5], 7, 1, 5)


@pytest.mark.parametrize("name,lost", [
    ("ec32", (0,)), ("ec32", (0, 2)), ("ec32", (1, 3)), ("xor3", (2,)),
    ("ec52", (4, 6))])
def test_write_chunks_degraded_host(name, lost):
    """Three chunks of 7, 5 and 2k+1 blocks, per-chunk block ranges, the
    parts in one [S, L] array each; parts as the slice numbers them."""
    from lizardfs_amd import chunkwrite as W
    sl = D.SLICES[name]
    t = slice_type(name)
    rsl = C.Slice(*sl.kind)
    n = [7, 5, 2 * sl.ks + 1]
    first, count = [1, 0, sl.ks - 1], [sl.ks + 1, sl.ks + 1, sl.ks + 1]
    frm, size = 4093, 8195
    rng = np.random.default_rng(23)
    chunks = [rng.integers(0, 256, (k, BLOCK), np.uint8) for k in n]
    room = 4
    frags = [np.zeros((3, room * BLOCK), np.uint8)
             for _ in range(rsl.nparts)]
    for s, chunk in enumerate(chunks):
        for p, part in enumerate(rsl.cut(chunk)):
            frags[p][s, :part.size] = part.reshape(-1)
    avail = [p for p in range(rsl.nparts) if p not in lost]
    given = [f if p in avail else None for p, f in enumerate(frags)]
    data = rng.integers(0, 256, (3, sl.ks + 1, size), np.uint8)
    parity, crcs, packets = W.write_chunks_degraded_host(
        t, given, n, data, first, count, avail, frm, size)
    for s, chunk in enumerate(chunks):
        after = np.zeros((max(n[s], first[s] + count[s]), BLOCK), np.uint8)
        after[:n[s]] = chunk
        after[first[s]:first[s] + count[s], frm:frm + size] = data[s]
        want = rsl.cut(after)
        plan = W.plan_write_degraded(t, avail, n[s], first[s], count[s])
        assert [(p.part, p.block) for p in packets[s]] == plan.packets
        assert all(p.part in avail for p in packets[s])
        assert {p.part for p in packets[s]} >= set(rsl.parity) & set(avail)
        for p in packets[s]:
            assert np.array_equal(p.data,
                                  want[p.part][p.block, frm:frm + size])
            assert p.crc == oracle.crc32(p.data)
    # availability per chunk gives the same
    again = W.write_chunks_degraded_host(t, given, n, data, first, count,
                                         [avail] * 3, frm, size)
    assert np.array_equal(again[0], parity) and np.array_equal(again[1], crcs)


SHORT = [  # slice, chunk blocks, first, count, available parts
    ("ec32", 4, 4, 1, [1, 2, 3, 4]),   # row 1: lost, new, absent
    ("ec32", 5, 5, 1, [0, 2, 3, 4]),   # row 1: fill, lost, new
    ("ec32", 4, 4, 1, [1, 2, 4]),      # parity 0 lost as well
    ("ec32", 2, 7, 1, [2, 3, 4]),      # wholly past the end
    ("xor3", 4, 4, 1, [0, 2, 3]),      # xor parts: column 0 is part 1
    ("ec52", 7, 8, 1, [0, 2, 3, 4, 6])]   # fill, lost, absent, new, absent


def short_chunk_case(name, n, first, count, avail, frm=4093, size=8195):
    """One short chunk whose survivors do not all reach the touched row:
    (slice type, fragments with None for lost parts, data, expected parts
    after the write)."""
    sl = C.Slice(*D.SLICES[name].kind)
    rng = np.random.default_rng(31)
    chunk = rng.integers(0, 256, (n, BLOCK), np.uint8)
    frags = [np.zeros((1, 4 * BLOCK), np.uint8) if p in avail else None
             for p in range(sl.nparts)]
    for p, part in enumerate(sl.cut(chunk)):
        if p in avail:
            frags[p][0, :part.size] = part.reshape(-1)
    data = rng.integers(0, 256, (1, count, size), np.uint8)
    after = np.zeros((max(n, first + count), BLOCK), np.uint8)
    after[:n] = chunk
    after[first:first + count, frm:frm + size] = data[0]
    return slice_type(name), frags, data, sl.cut(after)


def check_short_chunk_packets(t, packets, want, n, first, count, avail,
                              frm=4093, size=8195):
    from lizardfs_amd import chunkwrite as W
    plan = W.plan_write_degraded(t, avail, n, first, count)
    assert [(p.part, p.block) for p in packets] == plan.packets
    assert packets and all(p.part in avail for p in packets)
    for p in packets:
        got = p.data if isinstance(p.data, np.ndarray) else \
            p.data.cpu().numpy()
        assert np.array_equal(got, want[p.part][p.block, frm:frm + size])
        assert p.crc == oracle.crc32(got)


@pytest.mark.parametrize("name,n,first,count,avail", SHORT)
def test_write_chunks_degraded_host_single_short_chunk(name, n, first, count,
                                                       avail):
    """The slots are the parts the plan reads, and the plan leaves out a
    survivor that does not reach the row: the table must not ask for it."""
    from lizardfs_amd import chunkwrite as W
    t, frags, data, want = short_chunk_case(name, n, first, count, avail)
    plan = W.plan_write_degraded(t, avail, n, first, count)
    assert W.LOST in [k for _, row in plan.rows for k in row] or \
        name == "ec32" and n == 2
    _, _, (packets,) = W.write_chunks_degraded_host(
        t, frags, [n], data, first, count, avail, 4093, 8195)
    check_short_chunk_packets(t, packets, want, n, first, count, avail)


def test_write_chunks_degraded_host_refusals():
    from lizardfs_amd import chunkwrite as W
    t = slice_type("ec32")
    frags = [np.zeros((1, 4 * BLOCK), np.uint8) for _ in range(5)]
    data = np.zeros((1, 2, 100), np.uint8)
    ok = dict(slice_type=t, fragments=frags, chunk_blocks=[7], data=data,
              first_block=1, block_count=2, available_parts=[1, 2, 3, 4],
              offset=5, size=100)
    W.write_chunks_degraded_host(**ok)
    for kw in (dict(available_parts=[1, 4]),          # unwritable
               dict(available_parts=[1, 2, 3, 5]),    # no such part
               dict(available_parts=[[1, 2, 3, 4]] * 2),
               dict(fragments=frags[:3] + [None] + frags[4:]),  # a survivor
               dict(offset=65500),
               dict(want_parity=[2]),
               dict(block_count=0)):
        with pytest.raises(ValueError):
            W.write_chunks_degraded_host(**{**ok, **kw})
    # the lost part's own fragment is not needed
    W.write_chunks_degraded_host(**{**ok, "fragments": [None] + frags[1:]})
