"""replicate_stream's argument checks (no GPU): every malformed call raises
ValueError before an engine is created or the pipeline entered, and the
arrays it was given are left as they were.

The base call is a valid ec(3,2) one, parts of one block, 2 chunks, erased
(1, 3); each case changes exactly one thing about it."""
import numpy as np
import pytest

from lizardfs_amd import lib as L
from lizardfs_amd import replicate
from lizardfs_amd import scrub
from lizardfs_amd import slice_traits as st

K, M, S = 3, 2, 2
PLEN = st.BLOCK_SIZE
ERASED = (1, 3)
HDR = scrub.header_size(st.ec_slice_type(K, M))
IMG = {"moosefs": HDR + PLEN, "interleaved": scrub.HDD_BLOCK}


@pytest.fixture(autouse=True)
def no_engine(monkeypatch):
    """A check that comes too late reaches the engine or the pipeline: fail
    there, with something that is not a ValueError."""
    def refuse(*a, **kw):
        raise AssertionError("the call got past replicate_stream's checks")
    monkeypatch.setattr(L, "engine", refuse)
    real = L.lib()

    class Guarded:
        lizec_replicate_run = staticmethod(refuse)
        lizec_replicate_run_interleaved = staticmethod(refuse)

        def __getattr__(self, name):
            return getattr(real, name)
    monkeypatch.setattr(L, "lib", lambda: Guarded())


def base(fmt="moosefs"):
    parts = [None if i in ERASED else np.full((S, PLEN), 0x11 * (i + 1),
                                              np.uint8)
             for i in range(K + M)]
    out = {p: np.full((S, IMG[fmt]), 0xA5, np.uint8) for p in ERASED}
    return dict(k=K, m=M, host_parts=parts, erased=ERASED, want=ERASED,
                chunk_ids=[1, 2], version=3, out=out, fmt=fmt)


def strided_cols(rows, cols):
    """[rows, cols] uint8 with inner stride 2."""
    a = np.full((rows, 2 * cols), 0xA5, np.uint8)[:, ::2]
    assert a.shape == (rows, cols) and a.strides[1] == 2
    return a


def wrong_slots(c):
    c["host_parts"] = c["host_parts"][:-1]


def erased_count(c):
    c["erased"] = (1,)


def want_outside(c):
    c["want"] = (1, 2)


def survivor_none(c):
    c["host_parts"][0] = None


def not_uint8(c):
    c["host_parts"][2] = c["host_parts"][2].view(np.int8)


def not_2d(c):
    c["host_parts"][2] = c["host_parts"][2].reshape(S, PLEN, 1)


def shapes_differ(c):
    c["host_parts"][4] = np.zeros((S + 1, PLEN), np.uint8)


def not_whole_blocks(c):
    c["host_parts"] = [None if a is None else a[:, :PLEN - 16]
                       for a in c["host_parts"]]


def chunk_id_count(c):
    c["chunk_ids"] = [1, 2, 3]


def unknown_fmt(c):
    c["fmt"] = "tape"


def out_shape(c):
    c["out"][3] = np.full((S, IMG[c["fmt"]] + 4), 0xA5, np.uint8)


def out_missing(c):
    del c["out"][3]


def part_inner_stride(c):
    c["host_parts"][2] = strided_cols(S, PLEN)


def out_inner_stride(c):
    c["out"][1] = strided_cols(S, IMG[c["fmt"]])


def part_negative_rows(c):
    c["host_parts"][0] = c["host_parts"][0][::-1]


def out_negative_rows(c):
    c["out"][3] = c["out"][3][::-1]


CASES = [wrong_slots, erased_count, want_outside, survivor_none, not_uint8,
         not_2d, shapes_differ, not_whole_blocks, chunk_id_count,
         unknown_fmt, out_shape, out_missing, part_inner_stride,
         out_inner_stride, part_negative_rows, out_negative_rows]


@pytest.mark.parametrize("fmt", ("moosefs", "interleaved"))
@pytest.mark.parametrize("spoil", CASES, ids=lambda f: f.__name__)
def test_refused(spoil, fmt):
    c = base(fmt)
    spoil(c)
    outs = list(c["out"].values())
    with pytest.raises(ValueError):
        replicate.replicate_stream(**c)
    for a in outs:
        assert (a == 0xA5).all(), "an output array was written"


@pytest.mark.parametrize("fmt", ("moosefs", "interleaved"))
def test_base_call_passes_the_checks(fmt):
    """The base call itself is refused by nothing: it reaches the pipeline
    (which the fixture replaces), so every case above fails for its own
    reason.  Row-strided arrays, rows further apart than their length, are
    legal on both sides."""
    c = base(fmt)
    with pytest.raises(AssertionError, match="got past"):
        replicate.replicate_stream(**c)
    c = base(fmt)
    wide = np.zeros((S, PLEN + 512), np.uint8)
    c["host_parts"][0] = wide[:, 256:256 + PLEN]
    wide_out = np.zeros((S, IMG[fmt] + 512), np.uint8)
    c["out"][1] = wide_out[:, 256:256 + IMG[fmt]]
    with pytest.raises(AssertionError, match="got past"):
        replicate.replicate_stream(**c)
