"""The host-only companions of lizec_replicate_run_ragged (no GPU): the stage
cut, lizec_replicate_ragged_stages, and the argument checks,
lizec_impl_replicate_ragged_check, one refusal per case, each changing one
thing in a valid call."""
import ctypes

import numpy as np
import pytest

import replicate_ragged_cases as C

from lizardfs_amd import lib as L
from lizardfs_amd import replicate

EINVAL = -2
u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)


def prepared(fmt="moosefs", want=None):
    pop = C.base()
    return replicate._stream_ragged_prepare(
        pop.k, pop.m, pop.sources(), pop.chunk_blocks, C.PER_CHUNK, want,
        pop.chunk_ids, C.VERSION, None, None, fmt)


def cut(p, stage_bytes, dst=None, cap=None, fmt_flags=None, count_only=False):
    S, oc = p["dst_nb"].shape
    if dst is None:
        dst = np.where(p["slots"] >= 0, 1, 0).astype(np.uint64)
    dst = np.ascontiguousarray(dst, np.uint64)
    cap = S + 1 if cap is None else cap
    first = np.full(max(cap, 1) + 1, 0xDEAD, np.uint32)
    n = L.lib().lizec_replicate_ragged_stages(
        p["src_nb"].shape[1], oc, p["src_nb"].ctypes.data_as(u32p),
        dst.ctypes.data_as(u64p), p["dst_nb"].ctypes.data_as(u32p), S,
        p["head"], p["flags"] if fmt_flags is None else fmt_flags,
        stage_bytes, None if count_only else first.ctypes.data_as(u32p), cap)
    if n < 0 or count_only:
        return n
    assert first[cap] == 0xDEAD, "wrote past cap"
    return first[:n + 1].tolist()


def footprint(p, dst_used=None):
    used = p["slots"] >= 0 if dst_used is None else dst_used
    img = np.where(used, (p["sizes"] + 15) & ~15, 0)
    return p["src_nb"].astype(np.int64).sum(axis=1) * C.BLOCK + img.sum(axis=1)


def test_one_stage_when_everything_fits():
    p = prepared()
    assert cut(p, 0) == [0, 6]
    assert cut(p, int(footprint(p).sum())) == [0, 6]
    assert cut(p, 0, count_only=True) == 1


def test_boundary_at_exactly_two_chunks():
    p = prepared()
    f = footprint(p)
    two = int(f[0] + f[1])
    assert cut(p, two)[:2] == [0, 2]          # chunks 0 and 1 just fit
    assert cut(p, two - 1)[:3] == [0, 1, 2]   # one byte less: chunk 1 moves on


def test_every_chunk_oversized():
    p = prepared()
    assert cut(p, 1) == [0, 1, 2, 3, 4, 5, 6]
    assert cut(p, int(footprint(p).min()) - 1) == [0, 1, 2, 3, 4, 5, 6]


def test_unwanted_slot_does_not_count():
    """want of one part in some chunks: the unused slot (address 0) adds
    nothing; neither does a slot whose address is 0 although a part is named
    for it."""
    want = [(0, 3), (4,), (3, 4), (0,), (2, 4), (2,)]
    p = prepared(want=want)
    full = prepared()
    f, ffull = footprint(p), footprint(full)
    assert f[1] < ffull[1] and f[0] == ffull[0]
    two = int(f[0] + f[1])
    assert cut(p, two)[:2] == [0, 2] and cut(p, two - 1)[:3] == [0, 1, 2]
    # drop chunk 0's second image as well: it fits where it did not before
    dst = np.where(p["slots"] >= 0, 1, 0)
    dst[0, 1] = 0
    used = dst != 0
    f2 = footprint(p, used)
    assert f2[0] < f[0]
    assert cut(p, int(f2[0] + f2[1]), dst=dst)[:2] == [0, 2]
    assert cut(p, int(f2[0] + f2[1]))[:3] == [0, 1, 2]


def test_formats_have_their_own_footprints():
    pm, pi = prepared("moosefs"), prepared("interleaved")
    fm, fi = footprint(pm), footprint(pi)
    # ec(3,2) headers are 4096 bytes, an INTERLEAVED block carries 4
    assert (fm > fi).all()
    two = int(fi[0] + fi[1])
    assert cut(pi, two)[:2] == [0, 2]
    assert cut(pm, two)[:3] == [0, 1, 2]
    # an INTERLEAVED image of no blocks is nothing: header_size is not counted
    p = prepared("interleaved")
    p["head"] = 4096
    assert cut(p, two)[:2] == [0, 2]


def test_cap_too_small_is_refused():
    p = prepared()
    assert cut(p, 1, cap=7) == [0, 1, 2, 3, 4, 5, 6]
    assert cut(p, 1, cap=6) == EINVAL
    assert cut(p, 0, cap=1) == EINVAL
    assert cut(p, 0, cap=2) == [0, 6]


def test_stage_refusals():
    p = prepared()
    assert cut(p, (1 << 31) + 1) == EINVAL
    assert cut(p, 1 << 31) == [0, 6]
    assert cut(p, 0, fmt_flags=2) == EINVAL
    q = dict(p, src_nb=p["src_nb"].copy())
    q["src_nb"][2, 0] = 1025
    assert cut(q, 0) == EINVAL


# ---------------------------------------------------------------------------
# lizec_impl_replicate_ragged_check


def valid_call(fmt="moosefs"):
    """The arguments of a valid verified call over the base population, with
    the arrays that back them."""
    pop = C.base()
    p = replicate._stream_ragged_prepare(
        pop.k, pop.m, pop.sources(), pop.chunk_blocks, C.PER_CHUNK, None,
        pop.chunk_ids, C.VERSION, pop.source_crcs(), None, fmt)
    S, oc = p["dst_nb"].shape
    return dict(
        ic=pop.k, oc=oc, gftbls=p["tables"].copy(), ntables=p["tables"].shape[0],
        tbl_index=p["index"].copy(), host_src=p["src"].copy(),
        src_nblocks=p["src_nb"].copy(),
        host_src_crc=np.ascontiguousarray(p["src_crc"]).copy(),
        sigs=p["sigs"].copy(), sig_len=22, header_size=p["head"] or 4096,
        crc_off=1024, host_dst=np.full((S, oc), 0x1000, np.uint64),
        dst_nblocks=p["dst_nb"].copy(), nchunks=S, stage_bytes=0,
        flags=p["flags"], bad_out=np.zeros(S, np.uint32))


def check(c):
    def ptr(a, t):
        return None if a is None else np.ascontiguousarray(a).ctypes.data_as(t)
    keep = {k: np.ascontiguousarray(v) for k, v in c.items()
            if isinstance(v, np.ndarray)}
    return L.lib().lizec_impl_replicate_ragged_check(
        c["ic"], c["oc"], ptr(keep.get("gftbls"), u8p), c["ntables"],
        ptr(keep.get("tbl_index"), u32p), ptr(keep.get("host_src"), u64p),
        ptr(keep.get("src_nblocks"), u32p),
        ptr(keep.get("host_src_crc"), u64p), ptr(keep.get("sigs"), u8p),
        c["sig_len"], c["header_size"], c["crc_off"],
        ptr(keep.get("host_dst"), u64p), ptr(keep.get("dst_nblocks"), u32p),
        c["nchunks"], c["stage_bytes"], c["flags"],
        ptr(keep.get("bad_out"), u32p))


def null(name):
    def f(c):
        c[name] = None
    f.__name__ = f"null_{name}"
    return f


def setv(name, value, label=None):
    def f(c):
        c[name] = value
    f.__name__ = label or f"{name}_{value}"
    return f


def tbl_index_out_of_range(c):
    c["tbl_index"][4] = c["ntables"]


def ntables_too_large(c):
    # the multi call's limit: ntables * 32 * ic * oc <= 2^30; the table
    # pointer is not followed by the check
    c["ntables"] = (1 << 30) // (32 * c["ic"] * c["oc"]) + 1
    c["tbl_index"] = None


def src_count_above_1024(c):
    c["src_nblocks"][5, 2] = 1025


def dst_count_above_1024(c):
    c["dst_nblocks"][5, 0] = 1025


def src_count_without_address(c):
    c["host_src"][3, 1] = 0


def dst_count_without_address(c):
    c["host_dst"][5, 1] = 0


def crc_array_does_not_fit(c):
    c["crc_off"] = c["header_size"] - 4 * int(c["dst_nblocks"].max()) + 1


REFUSALS = [
    null("gftbls"), null("host_src"), null("src_nblocks"), null("host_dst"),
    null("dst_nblocks"), null("bad_out"),
    setv("nchunks", 0), setv("ic", 0), setv("ic", 33), setv("oc", 0),
    setv("oc", 33), tbl_index_out_of_range, setv("ntables", 0),
    ntables_too_large, src_count_above_1024, dst_count_above_1024,
    src_count_without_address, dst_count_without_address,
    setv("header_size", 4088), setv("sig_len", 4097),
    crc_array_does_not_fit, setv("flags", 2, "unknown_flag"),
    setv("flags", 3, "unknown_flag_with_known"),
    setv("stage_bytes", (1 << 31) + 1, "stage_bytes_above_2g"),
]


@pytest.mark.parametrize("spoil", REFUSALS, ids=lambda f: f.__name__)
def test_check_refuses(spoil):
    c = valid_call()
    assert check(c) == 0
    spoil(c)
    assert check(c) == EINVAL


def test_check_accepts_the_legal_edges():
    c = valid_call()
    c["stage_bytes"] = 1 << 31
    assert check(c) == 0
    # no verification: bad_out may be NULL, and so may tbl_index and sigs
    c["host_src_crc"] = c["bad_out"] = c["tbl_index"] = c["sigs"] = None
    c["ntables"] = 1
    assert check(c) == 0
    # a count of 0 needs no address, on either side
    c = valid_call()
    zs = np.argwhere(c["src_nblocks"] == 0)
    assert len(zs)
    c["host_src"][tuple(zs[0])] = 0
    c["dst_nblocks"][0, 1] = 0
    c["host_dst"][0, 1] = 0
    assert check(c) == 0
    # a count of exactly 1024 is legal where the CRC array holds it
    c["src_nblocks"][tuple(np.argwhere(c["src_nblocks"] > 0)[0])] = 1024
    assert check(c) == 0
    # INTERLEAVED: the header arguments are unused
    c = valid_call("interleaved")
    c["header_size"], c["sig_len"], c["crc_off"] = 7, 99, 1 << 20
    assert check(c) == 0


def test_host_twin_makes_the_same_checks():
    """lizec_replicate_ragged_host goes through the check: a refused call
    writes nothing."""
    c = valid_call()
    arena = np.full(64, C.FILL, np.uint8)
    c["host_dst"][:] = arena.ctypes.data
    c["flags"] = 2
    keep = {k: np.ascontiguousarray(v) for k, v in c.items()
            if isinstance(v, np.ndarray)}
    r = L.lib().lizec_replicate_ragged_host(
        c["ic"], c["oc"], keep["gftbls"].ctypes.data_as(u8p), c["ntables"],
        keep["tbl_index"].ctypes.data_as(u32p),
        keep["host_src"].ctypes.data_as(u64p),
        keep["src_nblocks"].ctypes.data_as(u32p),
        keep["host_src_crc"].ctypes.data_as(u64p),
        keep["sigs"].ctypes.data_as(u8p), c["sig_len"], c["header_size"],
        c["crc_off"], keep["host_dst"].ctypes.data_as(u64p),
        keep["dst_nblocks"].ctypes.data_as(u32p), c["nchunks"], c["flags"],
        keep["bad_out"].ctypes.data_as(u32p))
    assert r == EINVAL
    assert (arena == C.FILL).all()
