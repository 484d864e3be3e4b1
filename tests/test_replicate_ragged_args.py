"""replicate_stream_ragged's argument checks (no GPU): every malformed call
raises ValueError before an engine is created or the pipeline entered, and
the arrays it was given are left as they were.

The base call is the valid verified one of replicate_ragged_cases.py — ec(3,2),
six chunks of 1..7 blocks, a pattern per chunk — and each case changes exactly
one thing about it."""
import numpy as np
import pytest

import replicate_ragged_cases as C

from lizardfs_amd import lib as L
from lizardfs_amd import replicate


@pytest.fixture(autouse=True)
def no_engine(monkeypatch):
    """A check that comes too late reaches the engine or the pipeline: fail
    there, with something that is not a ValueError."""
    def refuse(*a, **kw):
        raise AssertionError("the call got past replicate_stream_ragged's "
                             "checks")
    monkeypatch.setattr(L, "engine", refuse)
    monkeypatch.setattr(L, "pinned_empty", refuse)
    real = L.lib()

    class Guarded:
        lizec_replicate_run_ragged = staticmethod(refuse)
        lizec_replicate_ragged_host = staticmethod(refuse)

        def __getattr__(self, name):
            return getattr(real, name)
    monkeypatch.setattr(L, "lib", lambda: Guarded())


def base(fmt="moosefs"):
    pop = C.base()
    out = {}
    for s, w in enumerate(C.PER_CHUNK):
        for p in w:
            out[(s, p)] = np.full(pop.image_size(s, p, fmt), C.FILL, np.uint8)
    return dict(k=pop.k, m=pop.m, host_parts=pop.sources(),
                chunk_blocks=list(pop.chunk_blocks),
                erased=[tuple(e) for e in C.PER_CHUNK], want=None,
                chunk_ids=list(pop.chunk_ids), version=C.VERSION,
                crcs=pop.source_crcs(), out=out, fmt=fmt)


def wrong_slots(c):
    c["host_parts"] = c["host_parts"][:-1]


def erased_count(c):
    c["erased"][2] = (3,)


def erased_entries(c):
    c["erased"] = c["erased"][:-1]


def want_outside(c):
    c["want"] = [tuple(e) for e in c["erased"]]
    c["want"][1] = (1, 2)


def survivor_none(c):
    c["host_parts"][0] = None


def not_uint8(c):
    c["host_parts"][2] = c["host_parts"][2].view(np.int8)


def not_2d(c):
    a = c["host_parts"][2]
    c["host_parts"][2] = a.reshape(a.shape[0], a.shape[1], 1)


def rows_differ(c):
    c["host_parts"][4] = np.zeros((7, c["host_parts"][4].shape[1]), np.uint8)


def rows_too_short(c):
    # part 0 has 3 blocks in the 7-block chunk
    c["host_parts"][0] = c["host_parts"][0][:, :3 * C.BLOCK - 16]


def part_inner_stride(c):
    a = c["host_parts"][2]
    wide = np.zeros((a.shape[0], 2 * a.shape[1]), np.uint8)
    c["host_parts"][2] = wide[:, ::2]


def part_negative_rows(c):
    c["host_parts"][0] = c["host_parts"][0][::-1]


def blocks_zero(c):
    c["chunk_blocks"][0] = 0


def blocks_above_1024(c):
    c["chunk_blocks"][5] = 1025


def blocks_not_int(c):
    c["chunk_blocks"] = [float(n) for n in c["chunk_blocks"]]


def blocks_2d(c):
    c["chunk_blocks"] = [c["chunk_blocks"]]


def chunk_id_count(c):
    c["chunk_ids"] = c["chunk_ids"] + [9]


def unknown_fmt(c):
    c["fmt"] = "tape"


def crcs_slots(c):
    c["crcs"] = c["crcs"][:-1]


def crcs_dtype(c):
    a = c["crcs"][2]
    c["crcs"][2] = np.ascontiguousarray(a).view("<u4").reshape(a.shape[:2])


def crcs_rows(c):
    c["crcs"][2] = c["crcs"][2][:-1]


def crcs_too_few(c):
    c["crcs"][0] = c["crcs"][0][:, :2]


def crcs_strided(c):
    a = c["crcs"][2]
    wide = np.zeros((a.shape[0], 2 * a.shape[1], 4), np.uint8)
    c["crcs"][2] = wide[:, ::2]


def out_missing(c):
    del c["out"][(3, 1)]


def out_size(c):
    a = c["out"][(3, 1)]
    c["out"][(3, 1)] = np.full(a.size + 4, C.FILL, np.uint8)


def out_not_1d(c):
    a = c["out"][(3, 1)]
    c["out"][(3, 1)] = a.reshape(1, -1)


def out_strided(c):
    a = c["out"][(3, 1)]
    c["out"][(3, 1)] = np.full(2 * a.size, C.FILL, np.uint8)[::2]


def out_dtype(c):
    c["out"][(3, 1)] = c["out"][(3, 1)].view(np.int8)


def stage_bytes_too_large(c):
    c["stage_bytes"] = (1 << 31) + 1


CASES = [wrong_slots, erased_count, erased_entries, want_outside,
         survivor_none, not_uint8, not_2d, rows_differ, rows_too_short,
         part_inner_stride, part_negative_rows, blocks_zero,
         blocks_above_1024, blocks_not_int, blocks_2d, chunk_id_count,
         unknown_fmt, crcs_slots, crcs_dtype, crcs_rows, crcs_too_few,
         crcs_strided, out_missing, out_size, out_not_1d, out_strided,
         out_dtype, stage_bytes_too_large]


# chunk ids are unused in INTERLEAVED format, so their number is not checked
REFUSED = [(f, fmt) for fmt in C.FORMATS for f in CASES
           if not (f is chunk_id_count and fmt == "interleaved")]


@pytest.mark.parametrize("spoil,fmt", REFUSED,
                         ids=[f"{f.__name__}-{fmt}" for f, fmt in REFUSED])
def test_refused(spoil, fmt):
    c = base(fmt)
    spoil(c)
    outs = list(c["out"].values())
    with pytest.raises(ValueError):
        replicate.replicate_stream_ragged(**c)
    for a in outs:
        assert (a.view(np.uint8) == C.FILL).all(), "an output was written"


@pytest.mark.parametrize("spoil", [c for c in CASES
                                   if c is not stage_bytes_too_large],
                         ids=lambda f: f.__name__)
def test_host_twin_refuses_the_same(spoil):
    c = base()
    spoil(c)
    with pytest.raises(ValueError):
        replicate.replicate_stream_ragged_host(**c)


@pytest.mark.parametrize("fmt", C.FORMATS)
def test_base_call_passes_the_checks(fmt):
    """The base call itself is refused by nothing: it reaches the engine
    (which the fixture replaces), so every case above fails for its own
    reason.  Row-strided arrays, a part that is lost everywhere given as
    None, and CRCs as big-endian words are legal."""
    with pytest.raises(AssertionError, match="got past"):
        replicate.replicate_stream_ragged(**base(fmt))
    with pytest.raises(AssertionError, match="got past"):
        replicate.replicate_stream_ragged_host(**base(fmt))
    c = base(fmt)
    a = c["host_parts"][0]
    wide = np.zeros((a.shape[0], a.shape[1] + 512), np.uint8)
    c["host_parts"][0] = wide[:, 256:256 + a.shape[1]]
    b = c["crcs"][4]
    c["crcs"][4] = np.ascontiguousarray(b).view(">u4").reshape(b.shape[:2])
    c["crcs"][1] = None
    with pytest.raises(AssertionError, match="got past"):
        replicate.replicate_stream_ragged(**c)
    # one pattern for all chunks: the lost parts need no array
    c = base(fmt)
    c["erased"] = (0, 3)
    c["host_parts"][0] = c["host_parts"][3] = None
    pop = C.base()
    c["out"] = {(s, p): np.zeros(pop.image_size(s, p, fmt), np.uint8)
                for s in range(pop.S) for p in (0, 3)}
    with pytest.raises(AssertionError, match="got past"):
        replicate.replicate_stream_ragged(**c)
