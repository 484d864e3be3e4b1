"""lizec_write_gate_host — hdd_write's data check, block check and CRC splice
(hddspacemgr.cc:1918-2001) over host memory — against a Python restatement
on the oracle (gate_cases.restate) and, for every accepted write, zlib's CRC
of the block with the data written into it.  CPU-only.

  sweep      twelve (offset, size) pairs x good data, wrong claimed CRC, no
             block, a flipped byte in each non-empty region of the block
  sparse     zero / non-zero block x stored 0 / empty-block CRC x flag
  refusals   every LIZEC_EINVAL of lizec.h, outputs left as they were
"""
import ctypes

import numpy as np
import pytest

import gate_cases as G
from lizardfs_amd import lib as L
from lizardfs_amd import writegate as wg

LIZEC_EINVAL = -2


def place(cases):
    """Ops over host memory for the cases; returns (ops, keepalive)."""
    ops = np.zeros(len(cases), wg.OP_DTYPE)
    keep = []
    for i, c in enumerate(cases):
        # data at every alignment 0..15, nothing behind its last byte
        pad = i % 16
        buf = np.zeros(pad + c.size, np.uint8)
        buf[pad:] = c.data
        stored = c.stored_bytes()
        keep += [buf, stored]
        ops[i]["data"] = buf.ctypes.data + pad if c.size else 0
        if c.block is not None:
            blk = np.ascontiguousarray(c.block).copy()
            keep.append(blk)
            ops[i]["block"] = blk.ctypes.data
            ops[i]["stored"] = stored.ctypes.data
        ops[i]["offset"], ops[i]["size"] = c.offset, c.size
        ops[i]["crc"] = c.claimed
    return ops, keep


def check(cases, sparse):
    ops, keep = place(cases)
    status, newcrc = wg.gate_host(ops, sparse=sparse)
    for i, c in enumerate(cases):
        exp = c.expect(sparse)
        assert (int(status[i]), int(newcrc[i])) == exp, \
            f"{c.name} (sparse={sparse}): got status {status[i]} " \
            f"newcrc {int(newcrc[i]):#010x}, expected {exp[0]} {exp[1]:#010x}"
        if exp[0] == G.OK:
            assert int(newcrc[i]) == G.spliced_crc(c.offset, c.size, c.data,
                                                   c.block), \
                f"{c.name}: new CRC is not that of the written block"
    return status


def test_op_struct_layout():
    assert wg.OP_DTYPE.itemsize == 40
    assert [wg.OP_DTYPE.fields[f][1] for f in
            ("data", "block", "stored", "offset", "size", "crc",
             "reserved")] == [0, 8, 16, 24, 28, 32, 36]


@pytest.mark.parametrize("sparse", (False, True))
def test_sweep(sparse):
    cases = G.sweep_cases()
    status = check(cases, sparse)
    # the matrix really holds all three outcomes, and a full-block write
    # ignores its block
    assert {G.OK, G.BAD_DATA, G.BAD_BLOCK} == set(int(s) for s in status)
    for i, c in enumerate(cases):
        if "flipped" in c.name:
            full = (c.offset, c.size) == (0, G.BLOCK)
            assert status[i] == (G.OK if full else G.BAD_BLOCK), c.name
        elif "wrong data crc" in c.name:
            assert status[i] == G.BAD_DATA, c.name
        else:
            assert status[i] == G.OK, c.name


def test_sparse_table():
    cases = G.sparse_cases()
    on = check(cases, True)
    off = check(cases, False)
    for i, c in enumerate(cases):
        zero = not c.block.any()
        empty = c.stored.any()          # stored = the empty-block CRC
        assert on[i] == (G.OK if zero else G.BAD_BLOCK), c.name
        assert off[i] == (G.OK if zero and empty else G.BAD_BLOCK), c.name


def test_full_block_ignores_block_and_stored():
    rng = np.random.default_rng(5)
    data = rng.integers(0, 256, G.BLOCK, np.uint8)
    op = np.zeros(1, wg.OP_DTYPE)
    op[0]["data"], op[0]["size"] = data.ctypes.data, G.BLOCK
    op[0]["crc"] = G.crc(data)
    op[0]["block"] = 1          # never dereferenced
    status, newcrc = wg.gate_host(op)
    assert (status[0], newcrc[0]) == (G.OK, G.crc(data))


def raw(ops, n, flags, status, newcrc):
    p = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None
    return L.lib().lizec_write_gate_host(p(ops), n, flags, p(status),
                                         p(newcrc))


def test_refusals_leave_outputs_untouched():
    cases = G.sweep_cases()[:4]
    good, keep = place(cases)
    blk = np.zeros(G.BLOCK, np.uint8)
    one = np.zeros(1, np.uint8)

    def broken(**fields):
        ops = good.copy()
        last = ops[-1]
        last["data"], last["block"] = one.ctypes.data, 0
        last["stored"] = 0
        last["offset"], last["size"], last["reserved"] = 0, 1, 0
        for k, v in fields.items():
            last[k] = v
        return ops

    n = good.size
    refused = [
        ("ops NULL", None, n, 0),
        ("n == 0", good, 0, 0),
        ("n > 2^24", good, (1 << 24) + 1, 0),
        ("size > 65536", broken(size=65537), n, 0),
        ("offset >= 65536", broken(offset=65536, size=0), n, 0),
        ("offset + size > 65536", broken(offset=65535, size=2), n, 0),
        ("reserved != 0", broken(reserved=1), n, 0),
        ("size > 0 with data == 0", broken(data=0), n, 0),
        ("partial op, block without stored",
         broken(block=blk.ctypes.data, stored=0), n, 0),
        ("unknown flag bit", good, n, 2),
        ("unknown high flag bit", good, n, 0x80000001),
    ]
    for what, ops, cnt, flags in refused:
        status = np.full(n, -77, np.int32)
        newcrc = np.full(n, 0xDEADBEEF, np.uint32)
        assert raw(ops, cnt, flags, status, newcrc) == LIZEC_EINVAL, what
        assert (status == -77).all() and (newcrc == 0xDEADBEEF).all(), what
    status = np.full(n, -77, np.int32)
    newcrc = np.full(n, 0xDEADBEEF, np.uint32)
    assert raw(good, n, 0, None, newcrc) == LIZEC_EINVAL
    assert raw(good, n, 0, status, None) == LIZEC_EINVAL
    assert (status == -77).all() and (newcrc == 0xDEADBEEF).all()
    # the unbroken template itself is accepted
    assert raw(broken(), n, 0, status, newcrc) == 0
    assert (status != -77).all()
    # and the python wrapper raises on a refusal
    with pytest.raises(L.LizecError):
        wg.gate_host(broken(reserved=1))
