"""The client read path — ChunkReader::readData (chunk_reader.cc:85-131) for
a batch of requests, in one lizec_chunk_read_batch call.

A read asks for chunk blocks [first_block, first_block + block_count).  The
slice's data parts interleave the chunk round-robin (ChunkReadPlanner,
chunk_read_planner.h:86-162); lost parts are rebuilt from the others
(ECReadPlan::recoverParts, ec_read_plan.h:113-146;
XorReadPlan::postProcessRead, xor_read_plan.h:77-126) and BlockConverter
(chunk_read_planner.h:36-58) puts part blocks back into chunk order.  The
kernel does the three in one pass: it copies the blocks of the surviving
columns and computes those of the lost ones from the same loaded registers,
so neither the parts nor the chunk are assembled in between.
"""
import collections
import ctypes

import numpy as np

from . import lib as L
from . import slice_traits as st
from .convert import (_check_slice, _part_blocks, _required_parts,
                      _total_parts, view_columns)

_BLOCK = st.BLOCK_SIZE
LOST = 0x80          # col_map: 0x80 + r = lost, table row r
UNMAPPED = 0xFF      # col_map: no requested block falls in the column

ReadPlan = collections.namedtuple("ReadPlan", "parts col_map lost")
ReadPlan.__doc__ = """What one read uses:
  parts   — the slice parts to read, ascending; part parts[j] is source j;
  col_map — per view column (convert.view_columns): j = source j, copied;
            LOST + r = rebuilt by table row r; UNMAPPED = not needed;
  lost    — the slice parts behind the lost columns, lost[r] for row r."""


def plan_read(slice_type, available_parts, first_block, block_count):
    """How the chunk planner would serve blocks [first_block, first_block +
    block_count) of a chunk from the parts of one slice, or None if it
    cannot (SliceReadPlanner::isReadingPossible, slice_read_planner.cc:46-51).
    If every required part (ChunkReadPlanner::getRequiredParts,
    chunk_read_planner.h:182-206) is available, only those are read.
    Otherwise an ec slice reads its first k available parts in ascending
    order (ec_read_plan.h:126-133) and a xor slice all its other parts, and
    the required parts that are missing are rebuilt.  Pure Python."""
    _check_slice(slice_type, "plan_read")
    if first_block < 0 or block_count < 1:
        raise ValueError("empty block range")
    nparts = _total_parts(slice_type)
    have = sorted({int(p) for p in available_parts})
    if have and not 0 <= have[0] <= have[-1] < nparts:
        raise ValueError(f"available part outside slice {slice_type}")
    cols = view_columns(slice_type)
    k = len(cols)
    required = _required_parts(slice_type, first_block, block_count)
    missing = sorted(p for p in required if p not in have)
    if not missing:
        parts = sorted(required)
    elif len(have) < k:
        return None
    else:
        # ec: the first k; xor: k = N others are all there is
        parts = have[:k]
    col_map = []
    for p in cols:
        if p in parts:
            col_map.append(parts.index(p))
        elif p in missing:
            col_map.append(LOST + missing.index(p))
        else:
            col_map.append(UNMAPPED)
    return ReadPlan(parts, col_map, missing)


def _per_chunk(v, S, what):
    a = np.asarray(v)
    if a.dtype.kind not in "iu" or a.ndim > 1:
        raise ValueError(f"{what} must be an int or one int per chunk")
    if a.ndim == 0:
        a = np.full(S, int(a))
    if a.size != S:
        raise ValueError(f"{what} has {a.size} entries for {S} chunks")
    return a.astype(np.int64)


class _Batch:
    """A checked batch of reads: the arrays of one lizec_chunk_read call,
    bar the tables (which need the library) and the destinations."""


def _prepare(slice_type, fragments, geom, chunk_blocks, first_block,
             block_count, erased, src_stride, dst_stride):
    """geom(fragment, what) -> (rows, row bytes, row stride, address), or
    ValueError.  Touches neither the library nor a GPU."""
    _check_slice(slice_type, "slice_type")
    cb = np.asarray(chunk_blocks)
    if cb.ndim != 1 or cb.size < 1 or cb.dtype.kind not in "iu":
        raise ValueError("chunk_blocks must be a 1-D int sequence")
    if cb.min() < 1 or cb.max() > st.BLOCKS_IN_CHUNK:
        raise ValueError(f"chunk_blocks out of [1, {st.BLOCKS_IN_CHUNK}]")
    S = cb.size
    for name, v in (("src_stride", src_stride), ("dst_stride", dst_stride)):
        if v < _BLOCK or v % 4:
            raise ValueError(f"{name}={v} must be a multiple of 4 and at "
                             f"least {_BLOCK}")
    first = _per_chunk(first_block, S, "first_block")
    count = _per_chunk(block_count, S, "block_count")
    if first.min() < 0 or count.min() < 1 or \
            (first + count).max() > st.BLOCKS_IN_CHUNK:
        raise ValueError(f"block ranges must be non-empty and inside "
                         f"[0, {st.BLOCKS_IN_CHUNK})")
    nparts = _total_parts(slice_type)
    fragments = list(fragments)
    if len(fragments) != nparts:
        raise ValueError(f"need {nparts} fragment slots for slice type "
                         f"{slice_type}")
    if erased is None:
        erased = [()] * S
    else:
        erased = list(erased)
        if all(isinstance(i, (int, np.integer)) for i in erased):
            erased = [erased] * S
        if len(erased) != S:
            raise ValueError(f"erased has {len(erased)} entries for {S} "
                             f"chunks")
    gone = []
    for s, e in enumerate(erased):
        e = sorted({int(i) for i in e})
        if e and not 0 <= e[0] <= e[-1] < nparts:
            raise ValueError(f"erased[{s}]: part index out of [0, {nparts})")
        gone.append(set(e))
    there = [p for p in range(nparts) if fragments[p] is not None]
    plans, seen = [], {}
    for s in range(S):
        # a batch repeats few patterns: plan each once
        key = (frozenset(gone[s]), int(first[s]), int(count[s]))
        if key not in seen:
            seen[key] = plan_read(
                slice_type, [p for p in there if p not in gone[s]],
                int(first[s]), int(count[s]))
        if seen[key] is None:
            raise ValueError(f"chunk {s}: blocks [{first[s]}, "
                             f"{first[s] + count[s]}) cannot be read from "
                             f"the parts that are left")
        plans.append(seen[key])
    counts = {int(n): [_part_blocks(slice_type, p, int(n))
                       for p in range(nparts)] for n in np.unique(cb)}
    src_nb = np.array([counts[int(n)] for n in cb], np.int64)
    bases = np.zeros(nparts, np.uint64)
    strides = np.zeros(nparts, np.uint64)
    for p in there:
        s, span, rstride, addr = geom(fragments[p], f"fragment {p}")
        if s != S:
            raise ValueError(f"fragment {p} has {s} rows, expected {S}")
        top = int(src_nb[:, p].max())
        need = (top - 1) * src_stride + _BLOCK if top else 0
        if span < need:
            raise ValueError(f"fragment {p}: rows of {span} bytes cannot "
                             f"hold {top} blocks at stride {src_stride} "
                             f"({need} bytes)")
        if addr % 4 or (s > 1 and rstride % 4):
            raise ValueError(f"fragment {p}: block data must be 4-byte "
                             f"aligned")
        bases[p], strides[p] = addr, rstride

    b = _Batch()
    b.S, b.slice_type, b.plans = S, slice_type, plans
    b.ks = st.data_parts(slice_type)
    b.srcs = b.ks          # ec: k survivors; xorN: the N others; standard: 1
    b.rows = max(len(p.lost) for p in plans)
    b.first, b.count = first.astype(np.uint32), count.astype(np.uint32)
    b.src_ptrs = np.zeros((S, b.srcs), np.uint64)
    b.src_nb = np.zeros((S, b.srcs), np.uint32)
    b.col_map = np.full((S, b.ks), UNMAPPED, np.uint8)
    for s, plan in enumerate(plans):
        for j, p in enumerate(plan.parts):
            # a part that holds no block of a short chunk keeps its address:
            # a requested column may be mapped to it and reads as zeros
            b.src_ptrs[s, j] = bases[p] + np.uint64(s) * strides[p]
            b.src_nb[s, j] = src_nb[s, p]
        b.col_map[s] = plan.col_map
    b.src_stride, b.dst_stride = src_stride, dst_stride
    b.need = (int(count.max()) - 1) * dst_stride + _BLOCK
    return b


def _tables(b):
    """(tables [P, 32*srcs*rows], index [S]) of a batch, one table per
    distinct (sources, lost parts) pattern; (None, None) without a loss."""
    if b.rows == 0:
        return None, None
    u8p = ctypes.POINTER(ctypes.c_uint8)
    keys, index = {}, np.zeros(b.S, np.uint32)
    for s, plan in enumerate(b.plans):
        if plan.lost:
            key = (tuple(plan.parts), tuple(plan.lost))
            index[s] = keys.setdefault(key, len(keys))
    tables = np.zeros((len(keys), 32 * b.srcs * b.rows), np.uint8)
    for (parts, lost), i in keys.items():
        if st.is_xor(b.slice_type):
            # all ones, as xor.py: the missing part is the XOR of the others
            tbl = np.zeros(32 * b.srcs, np.uint8)
            L.lib().ec_init_tables(
                b.srcs, 1, np.ones(b.srcs, np.uint8).ctypes.data_as(u8p),
                tbl.ctypes.data_as(u8p))
        else:
            from .ec import _pattern_table
            k, m = b.ks, st.parity_parts(b.slice_type)
            em = ((1 << (k + m)) - 1) & ~sum(1 << p for p in parts)
            tbl, rebuilt = _pattern_table(k, m, em, sum(1 << p for p in lost))
            assert tuple(rebuilt) == lost
        tables[i, :tbl.size] = tbl
    return tables, index


def _call(fn, head, b, dst, tail):
    u8p = ctypes.POINTER(ctypes.c_uint8)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    tables, index = _tables(b)
    dst = np.ascontiguousarray(dst, np.uint64)
    return fn(*head, b.srcs, b.rows,
              tables.ctypes.data_as(u8p) if b.rows else None,
              tables.shape[0] if b.rows else 0,
              index.ctypes.data_as(u32p) if b.rows else None,
              b.src_ptrs.ctypes.data_as(u64p), b.src_nb.ctypes.data_as(u32p),
              b.ks, b.col_map.ctypes.data_as(u8p),
              b.first.ctypes.data_as(u32p), b.count.ctypes.data_as(u32p),
              dst.ctypes.data_as(u64p), b.S, b.src_stride, b.dst_stride,
              *tail)


def read_chunks(slice_type, fragments, chunk_blocks, first_block,
                block_count, erased=None, out=None, src_stride=_BLOCK,
                dst_stride=_BLOCK, device=0):
    """Blocks [first_block, first_block + block_count) of a batch of chunks
    held as `slice_type` (standard, xorN or ec(k,m)), in one
    lizec_chunk_read_batch call.

    fragments: one [S, L] CUDA uint8 row view per part of the slice
      (standard: 1; xorN: N+1, part 0 the parity; ec(k,m): k+m), blocks at
      src_stride, or None for a part that is gone for every chunk.
    chunk_blocks: S block counts in 1..1024.  A requested block at or past
      a chunk's end comes out as zeros.
    first_block, block_count, erased (a set of missing parts): one value
      each, or one per chunk.  plan_read says what each read uses.
    out: optional [S, span] CUDA uint8 tensor with contiguous rows, blocks
      at dst_stride; the bytes between them are left alone.
    Returns out; of out[s] only the block_count[s] requested blocks are
    written.  Raises ValueError, before any GPU use, for what the library
    would refuse and for a read that the remaining parts cannot serve.
    """
    import torch

    def geom(t, what):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or \
                not t.is_cuda or t.dim() != 2 or t.stride(1) != 1:
            raise ValueError(f"{what} must be a CUDA uint8 [S, L] tensor "
                             f"with contiguous rows")
        return t.shape[0], t.shape[1], t.stride(0), t.data_ptr()

    b = _prepare(slice_type, fragments, geom, chunk_blocks, first_block,
                 block_count, erased, src_stride, dst_stride)
    if out is None:
        dev = next(t for t in fragments if t is not None).device
        out = torch.empty((b.S, b.need), dtype=torch.uint8, device=dev)
    else:
        s, span, rstride, addr = geom(out, "out")
        if s != b.S or span < b.need:
            raise ValueError(f"out must hold [S={b.S}, {b.need}] bytes")
        if addr % 4 or (s > 1 and rstride % 4):
            raise ValueError("out: block data must be 4-byte aligned")
    dst = np.uint64(out.data_ptr()) + \
        np.arange(b.S, dtype=np.uint64) * np.uint64(out.stride(0))
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    L.check(_call(L.lib().lizec_chunk_read_batch, (L.engine(device),), b,
                  dst, (stream,)), "lizec_chunk_read_batch")
    return out


def read_chunks_host(slice_type, fragments, chunk_blocks, first_block,
                     block_count, erased=None, out=None, src_stride=_BLOCK,
                     dst_stride=_BLOCK):
    """read_chunks over numpy arrays, through lizec_chunk_read_host: no GPU
    is needed.  fragments and out are uint8 [S, L] arrays with contiguous
    rows; a fresh out is zero-filled."""
    def geom(a, what):
        if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or \
                a.ndim != 2 or a.strides[1] != 1:
            raise ValueError(f"{what} must be a uint8 [S, L] array with "
                             f"contiguous rows")
        return a.shape[0], a.shape[1], a.strides[0], a.ctypes.data

    b = _prepare(slice_type, fragments, geom, chunk_blocks, first_block,
                 block_count, erased, src_stride, dst_stride)
    if out is None:
        out = np.zeros((b.S, b.need), np.uint8)
    else:
        s, span, rstride, addr = geom(out, "out")
        if s != b.S or span < b.need or not out.flags.writeable:
            raise ValueError(f"out must hold [S={b.S}, {b.need}] bytes")
        if addr % 4 or (s > 1 and rstride % 4):
            raise ValueError("out: block data must be 4-byte aligned")
    dst = np.uint64(out.ctypes.data) + \
        np.arange(b.S, dtype=np.uint64) * np.uint64(out.strides[0])
    L.check(_call(L.lib().lizec_chunk_read_host, (), b, dst, ()),
            "lizec_chunk_read_host")
    return out
