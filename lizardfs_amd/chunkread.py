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
             block_count, erased, src_stride, dst_stride, only=None):
    """geom(fragment, what) -> (rows, row bytes, row stride, address), or
    ValueError.  Touches neither the library nor a GPU.

    only: the chunks that the batch is to hold (a retry round of
    read_chunks_verified).  Everything is still checked for all S chunks,
    but a chunk of `only` that cannot be read is listed in .dead, not
    raised."""
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
    plans, seen, live, dead = [], {}, [], []
    for s in (range(S) if only is None else only):
        # a batch repeats few patterns: plan each once
        key = (frozenset(gone[s]), int(first[s]), int(count[s]))
        if key not in seen:
            seen[key] = plan_read(
                slice_type, [p for p in there if p not in gone[s]],
                int(first[s]), int(count[s]))
        if seen[key] is None and only is not None:
            dead.append(s)
            continue
        if seen[key] is None:
            raise ValueError(f"chunk {s}: blocks [{first[s]}, "
                             f"{first[s] + count[s]}) cannot be read from "
                             f"the parts that are left")
        plans.append(seen[key])
        live.append(s)
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

    # b.S reads, read i on chunk b.chunks[i]: all S chunks unless `only`
    b = _Batch()
    b.S, b.slice_type, b.plans = len(live), slice_type, plans
    b.chunks, b.dead, b.gone = live, dead, gone
    b.part_top = src_nb.max(axis=0)
    b.ks = st.data_parts(slice_type)
    b.srcs = b.ks          # ec: k survivors; xorN: the N others; standard: 1
    b.rows = max((len(p.lost) for p in plans), default=0)
    b.first = first[live].astype(np.uint32)
    b.count = count[live].astype(np.uint32)
    b.src_ptrs = np.zeros((b.S, b.srcs), np.uint64)
    b.src_nb = np.zeros((b.S, b.srcs), np.uint32)
    b.col_map = np.full((b.S, b.ks), UNMAPPED, np.uint8)
    for i, (s, plan) in enumerate(zip(live, plans)):
        for j, p in enumerate(plan.parts):
            # a part that holds no block of a short chunk keeps its address:
            # a requested column may be mapped to it and reads as zeros
            b.src_ptrs[i, j] = bases[p] + np.uint64(s) * strides[p]
            b.src_nb[i, j] = src_nb[s, p]
        b.col_map[i] = plan.col_map
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


# ---- the verified read -------------------------------------------------------

_INLINE = _BLOCK + 4    # [4-byte CRC][block]: INTERLEAVED images, READ_DATA

VerifiedRead = collections.namedtuple("VerifiedRead", "out corrupt unreadable")
VerifiedRead.__doc__ = """What read_chunks_verified returns:
  out        — as read_chunks;
  corrupt    — per chunk, the sorted tuple of parts that failed a CRC check
               (what the reference collects in crcErrors_);
  unreadable — per chunk, True where the parts that are left cannot serve
               the range; such a row's contents are unspecified."""


def _verified(slice_type, fragments, crcs, geom, chunk_blocks, first_block,
              block_count, erased, src_stride, dst_stride, inline_crcs,
              retry, make_out, run):
    """The rounds of a verified read over tensors or arrays.
    make_out(batch) -> (out, address of row 0, row stride);
    run(batch, dst, crc_ptrs, crc_stride) -> the masks, one per read, as a
    numpy array — it waits for them."""
    _check_slice(slice_type, "slice_type")
    nparts = _total_parts(slice_type)
    fragments = list(fragments)
    if inline_crcs:
        if crcs is not None:
            raise ValueError("inline_crcs: the CRCs lie in the fragments, "
                             "crcs must be None")
        if src_stride < _INLINE:
            raise ValueError(f"inline_crcs needs src_stride >= {_INLINE}")
        crcs = [None] * nparts

        def data_geom(t, what):
            s, span, rstride, addr = geom(t, what)
            return s, span - 4, rstride, addr + 4
    else:
        crcs = list(crcs) if crcs is not None else None
        if crcs is None or len(crcs) != nparts:
            raise ValueError(f"need {nparts} crcs entries (None = part not "
                             f"verified) for slice type {slice_type}")
        data_geom = geom
    args = (slice_type, fragments, data_geom, chunk_blocks, first_block,
            block_count)
    b = _prepare(*args, erased, src_stride, dst_stride)
    S = b.S
    # where the CRC of block 0 of part p of chunk s lies: base + s * stride
    crc_base = np.zeros(nparts, np.uint64)
    crc_rstride = np.zeros(nparts, np.uint64)
    for p in range(nparts):
        if inline_crcs and fragments[p] is not None:
            _, _, rstride, addr = geom(fragments[p], f"fragment {p}")
            crc_base[p], crc_rstride[p] = addr, rstride
        elif crcs[p] is not None:
            s, span, rstride, addr = geom(crcs[p], f"crcs[{p}]")
            if s != S or span < 4 * int(b.part_top[p]):
                raise ValueError(f"crcs[{p}] must hold [S={S}, "
                                 f"{4 * int(b.part_top[p])}] bytes")
            crc_base[p], crc_rstride[p] = addr, rstride
    crc_stride = src_stride if inline_crcs else 4
    out, out_addr, out_rstride = make_out(b)

    gone = [set(g) for g in b.gone]
    corrupt = [set() for _ in range(S)]
    unreadable = [False] * S
    while b.S:
        chunks = np.array(b.chunks, np.uint64)
        dst = np.uint64(out_addr) + chunks * np.uint64(out_rstride)
        crc_ptrs = np.zeros((b.S, b.srcs), np.uint64)
        for i, (s, plan) in enumerate(zip(b.chunks, b.plans)):
            for j, p in enumerate(plan.parts):
                if crc_base[p]:
                    crc_ptrs[i, j] = crc_base[p] + np.uint64(s) * crc_rstride[p]
        masks = run(b, dst, crc_ptrs, crc_stride)
        again = []
        for s, plan, mask in zip(b.chunks, b.plans, masks):
            if not mask:
                continue
            bad = [p for j, p in enumerate(plan.parts) if (int(mask) >> j) & 1]
            corrupt[s].update(bad)
            gone[s].update(bad)          # chunk_reader.cc:63-65
            if retry:
                again.append(s)
            else:
                unreadable[s] = True
        if not again:
            break
        b = _prepare(*args, gone, src_stride, dst_stride, only=again)
        for s in b.dead:
            unreadable[s] = True
    return VerifiedRead(out, [tuple(sorted(c)) for c in corrupt], unreadable)


def _verified_call(fn, head, b, dst, crc_ptrs, crc_stride, bad, tail):
    crc_ptrs = np.ascontiguousarray(crc_ptrs, np.uint64)
    return _call(fn, head, b, dst,
                 (crc_ptrs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                  crc_stride, bad) + tail)


def read_chunks_verified(slice_type, fragments, crcs, chunk_blocks,
                         first_block, block_count, erased=None, out=None,
                         src_stride=_BLOCK, dst_stride=_BLOCK,
                         inline_crcs=False, retry=True, device=0):
    """read_chunks with the client's CRC check and its retry: every source
    block a read consumes is compared with its CRC
    (lizec_chunk_read_verified_batch; read_operation_executor.cc:261-263),
    the parts that fail are dropped from the chunk's available parts
    (chunk_reader.cc:63-65), and the chunk is planned and read again from
    what is left.

    fragments, chunk_blocks, first_block, block_count, erased, out,
    src_stride, dst_stride: as read_chunks.
    crcs: one entry per part: None (the part is not verified) or a
      [S, >= 4*blocks] CUDA uint8 row view with the big-endian CRC of the
      part's block b at 4*b.
    inline_crcs: crcs must be None and src_stride >= 65540; every fragment
      row then starts at the CRC of block 0 — an INTERLEAVED part image's
      body, or readgate.read_packets output for whole blocks: block b's CRC
      at b*src_stride, its data at 4 + b*src_stride.
    retry: False = one round; a chunk with a bad part is then reported
      unreadable.

    Round 0 reads every chunk; each later round holds only the chunks whose
    last round found a bad part and that can still be planned, written to
    the same rows of out.  Every retried chunk has lost at least one more
    part, so there are at most as many rounds as the slice has parts.

    This function is SYNCHRONOUS: after each round it waits for the masks on
    the host, since the next round's plans depend on them.

    Returns VerifiedRead(out, corrupt, unreadable).  Raises ValueError,
    before any GPU use, for everything read_chunks raises it for (a read
    that the parts cannot serve before any check is one of them), for a
    crcs entry of the wrong shape, dtype, device or row count, and for
    inline_crcs with crcs given or a stride below 65540.
    """
    import torch

    def geom(t, what):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or \
                not t.is_cuda or t.dim() != 2 or t.stride(1) != 1:
            raise ValueError(f"{what} must be a CUDA uint8 [S, L] tensor "
                             f"with contiguous rows")
        return t.shape[0], t.shape[1], t.stride(0), t.data_ptr()

    def make_out(b):
        o = out
        if o is None:
            dev = next(t for t in fragments if t is not None).device
            o = torch.empty((b.S, b.need), dtype=torch.uint8, device=dev)
        else:
            s, span, rstride, addr = geom(o, "out")
            if s != b.S or span < b.need:
                raise ValueError(f"out must hold [S={b.S}, {b.need}] bytes")
            if addr % 4 or (s > 1 and rstride % 4):
                raise ValueError("out: block data must be 4-byte aligned")
        return o, o.data_ptr(), o.stride(0)

    def run(b, dst, crc_ptrs, crc_stride):
        bad = torch.empty(b.S, dtype=torch.int32,
                          device=torch.device("cuda", device))
        stream = ctypes.c_void_p(
            torch.cuda.current_stream(device).cuda_stream)
        L.check(_verified_call(
            L.lib().lizec_chunk_read_verified_batch, (L.engine(device),), b,
            dst, crc_ptrs, crc_stride, ctypes.c_void_p(bad.data_ptr()),
            (stream,)), "lizec_chunk_read_verified_batch")
        return bad.cpu().numpy().view(np.uint32)   # waits for the stream

    return _verified(slice_type, fragments, crcs, geom, chunk_blocks,
                     first_block, block_count, erased, src_stride,
                     dst_stride, inline_crcs, retry, make_out, run)


def read_chunks_verified_host(slice_type, fragments, crcs, chunk_blocks,
                              first_block, block_count, erased=None,
                              out=None, src_stride=_BLOCK, dst_stride=_BLOCK,
                              inline_crcs=False, retry=True):
    """read_chunks_verified over numpy arrays, through
    lizec_chunk_read_verified_host: no GPU is needed.  fragments, crcs and
    out are uint8 [S, L] arrays with contiguous rows; a fresh out is
    zero-filled."""
    def geom(a, what):
        if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or \
                a.ndim != 2 or a.strides[1] != 1:
            raise ValueError(f"{what} must be a uint8 [S, L] array with "
                             f"contiguous rows")
        return a.shape[0], a.shape[1], a.strides[0], a.ctypes.data

    def make_out(b):
        o = out
        if o is None:
            o = np.zeros((b.S, b.need), np.uint8)
        else:
            s, span, rstride, addr = geom(o, "out")
            if s != b.S or span < b.need or not o.flags.writeable:
                raise ValueError(f"out must hold [S={b.S}, {b.need}] bytes")
            if addr % 4 or (s > 1 and rstride % 4):
                raise ValueError("out: block data must be 4-byte aligned")
        return o, o.ctypes.data, o.strides[0]

    def run(b, dst, crc_ptrs, crc_stride):
        bad = np.zeros(b.S, np.uint32)
        L.check(_verified_call(
            L.lib().lizec_chunk_read_verified_host, (), b, dst, crc_ptrs,
            crc_stride, ctypes.c_void_p(bad.ctypes.data), ()),
            "lizec_chunk_read_verified_host")
        return bad

    return _verified(slice_type, fragments, crcs, geom, chunk_blocks,
                     first_block, block_count, erased, src_stride,
                     dst_stride, inline_crcs, retry, make_out, run)
