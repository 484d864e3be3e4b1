"""The client write path — ChunkWriter::startOperation
(mount/chunk_writer.cc:475-547) for a batch of writes, in one
lizec_chunk_write_batch call.

A write carries the bytes [offset, offset + size) of chunk blocks
[first_block, first_block + block_count).  The slice's data parts interleave
the chunk round-robin, so the range touches some block rows in part; the
columns of a touched row that the write does not cover are read back from
the parts (fillStripe, :440-466), columns past the chunk's end count as zeros
(:451), and the row's parities are computed over [offset, offset + size)
only (computeParityBlock, :365-402).  Every new data block and every parity
block leaves as a packet with the CRC of its bytes
(WriteExecutor::addDataPacket, write_executor.cc:91-107): exactly what
writegate checks on the other end.

A slice with lost parts is written through write_chunks_degraded, in one
lizec_chunk_write_degraded_batch call.  fillStripe reads a partly written
row through readBlocks (:557-615), a planned read over the parts that have
a location, so a fill column whose part is lost is rebuilt from the
survivors first.  Here rebuild and encode fold into one coefficient table
per row shape (lizec_degraded_write_table) over "new columns + old
sources", and the parity pass reads every needed byte range once; a lost
part gets no packets, neither data nor parity.
"""
import collections
import ctypes

import numpy as np

from . import lib as L
from . import scrub
from . import slice_traits as st
from .convert import _check_slice, _part_blocks, view_columns

_BLOCK = st.BLOCK_SIZE
NEW, FILL, ABSENT, LOST = "new", "fill", "absent", "lost"

# lizec_chunk_write: 40 bytes, no padding
WRITE_DTYPE = np.dtype([("data", "<u8"), ("crcs", "<u8"),
                        ("data_stride", "<u4"), ("par_stride", "<u4"),
                        ("first_block", "<u4"), ("block_count", "<u4"),
                        ("from", "<u4"), ("to", "<u4")])
assert WRITE_DTYPE.itemsize == 40

Packet = collections.namedtuple("Packet", "part block offset size crc data")
Packet.__doc__ = """The arguments of WriteExecutor::addDataPacket: `size`
bytes (`data`, a view of the caller's tensor or of the parity) for
[offset, offset + size) of block `block` of slice part `part`, and their
CRC."""

WritePlan = collections.namedtuple("WritePlan", "rows read_parts packets")
WritePlan.__doc__ = """What one write does:
  rows       — per touched block row: (row, [NEW | FILL | ABSENT per view
               column]);
  read_parts — the data parts that must be read back first, ascending;
  packets    — (part, block in part) of every packet in the reference's
               order: part by part, data parts then parity parts, ascending
               block."""


def _parity_parts(slice_type):
    cols = view_columns(slice_type)
    n = len(cols) + st.parity_parts(slice_type)
    return [p for p in range(n) if p not in cols]


def plan_write(slice_type, chunk_blocks, first_block, block_count):
    """How blocks [first_block, first_block + block_count) are written into
    a chunk that now holds chunk_blocks blocks of an xor or ec slice.  Pure
    Python."""
    _check_slice(slice_type, "plan_write")
    if st.parity_parts(slice_type) < 1:
        raise ValueError("plan_write: the slice has no parity part")
    if first_block < 0 or block_count < 1 or \
            first_block + block_count > st.BLOCKS_IN_CHUNK:
        raise ValueError(f"block range must be non-empty and inside "
                         f"[0, {st.BLOCKS_IN_CHUNK})")
    if not 0 <= chunk_blocks <= st.BLOCKS_IN_CHUNK:
        raise ValueError(f"chunk_blocks out of [0, {st.BLOCKS_IN_CHUNK}]")
    cols = view_columns(slice_type)
    ks = len(cols)
    end = first_block + block_count
    have = [_part_blocks(slice_type, p, chunk_blocks) for p in cols]
    rows, read = [], set()
    for b in range(first_block // ks, (end - 1) // ks + 1):
        kinds = []
        for c in range(ks):
            if first_block <= b * ks + c < end:
                kinds.append(NEW)
            elif b < have[c]:
                kinds.append(FILL)
                read.add(cols[c])
            else:
                kinds.append(ABSENT)
        rows.append((b, kinds))
    packets = []
    for c, p in enumerate(cols):
        packets += [(p, b) for b, kinds in rows if kinds[c] == NEW]
    for p in _parity_parts(slice_type):
        packets += [(p, b) for b, _ in rows]
    return WritePlan(rows, sorted(read), packets)


def _available(slice_type, available_parts, what):
    n = len(view_columns(slice_type)) + st.parity_parts(slice_type)
    have = sorted({int(p) for p in available_parts})
    if have and not 0 <= have[0] <= have[-1] < n:
        raise ValueError(f"{what}: available part outside slice "
                         f"{slice_type}")
    return have


def plan_write_degraded(slice_type, available_parts, chunk_blocks,
                        first_block, block_count):
    """plan_write for a slice of which only available_parts can be reached,
    or None if the write cannot be made.  Pure Python.

    rows carry a fourth kind, LOST: a fill column whose part is not
    available.  It is rebuilt, as ChunkWriter::readBlocks
    (chunk_writer.cc:557-615) does through the read planner, from the first
    k available parts in ascending order (ec_read_plan.h:126-133), for a
    xor slice from all the others; with fewer than k parts available the
    result is None ("Not enough chunkservers to read full data").
    read_parts are the old sources: the available fill parts, and for a row
    with a LOST column those k parts, bar data parts that do not reach the
    row (zeros).  packets holds the packets of available parts only: a lost
    part has no WriteExecutor, so neither its data packets nor its parity
    appear."""
    plan = plan_write(slice_type, chunk_blocks, first_block, block_count)
    have = _available(slice_type, available_parts, "plan_write_degraded")
    cols = view_columns(slice_type)
    ks = len(cols)
    blocks = {p: _part_blocks(slice_type, p, chunk_blocks) for p in have}
    rows, read = [], set()
    for b, kinds in plan.rows:
        kinds = [LOST if kind == FILL and cols[c] not in have else kind
                 for c, kind in enumerate(kinds)]
        rows.append((b, kinds))
        read.update(cols[c] for c, kind in enumerate(kinds) if kind == FILL)
        if LOST in kinds:
            if len(have) < ks:
                return None
            read.update(p for p in have[:ks] if b < blocks[p])
    packets = [(p, b) for p, b in plan.packets if p in have]
    return WritePlan(rows, sorted(read), packets)


def encode_table(slice_type):
    """The [rows][columns][32] table of a slice's parities: the encode table
    of ec(k,m), all ones for a xor slice (chunk_writer.cc:373-381)."""
    u8p = ctypes.POINTER(ctypes.c_uint8)
    ks, m = st.data_parts(slice_type), st.parity_parts(slice_type)
    tbl = np.zeros(32 * ks * m, np.uint8)
    if st.is_xor(slice_type):
        L.lib().ec_init_tables(ks, 1, np.ones(ks, np.uint8).ctypes.data_as(u8p),
                               tbl.ctypes.data_as(u8p))
    else:
        L.check(L.lib().lizec_rs_encode_tables(ks, m, tbl.ctypes.data_as(u8p)),
                "lizec_rs_encode_tables")
    return tbl


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
    """A checked batch of writes: the arrays of one lizec_chunk_write call,
    bar the table (which needs the library) and the outputs."""


def _prepare(slice_type, fragments, geom, chunk_blocks, data, first_block,
             block_count, offset, size, fmt, want_parity, available=None):
    """geom(buffer, what, dims) -> (shape, strides, address), or ValueError.
    Touches neither the library nor a GPU.  available: None, or the
    available parts of every chunk (the degraded call)."""
    _check_slice(slice_type, "slice_type")
    m = st.parity_parts(slice_type)
    if m < 1:
        raise ValueError("the slice has no parity part")
    cb = np.asarray(chunk_blocks)
    if cb.ndim != 1 or cb.size < 1 or cb.dtype.kind not in "iu":
        raise ValueError("chunk_blocks must be a 1-D int sequence")
    if cb.min() < 0 or cb.max() > st.BLOCKS_IN_CHUNK:
        raise ValueError(f"chunk_blocks out of [0, {st.BLOCKS_IN_CHUNK}]")
    S = cb.size
    if not (0 <= offset and 1 <= size and offset + size <= _BLOCK):
        raise ValueError(f"[offset, offset + size) must be a non-empty range "
                         f"inside [0, {_BLOCK})")
    first = _per_chunk(first_block, S, "first_block")
    count = _per_chunk(block_count, S, "block_count")
    if first.min() < 0 or count.min() < 1 or \
            (first + count).max() > st.BLOCKS_IN_CHUNK:
        raise ValueError(f"block ranges must be non-empty and inside "
                         f"[0, {st.BLOCKS_IN_CHUNK})")
    if fmt is None:
        data_off, bstride = 0, _BLOCK
    else:
        data_off, _, bstride, _ = scrub.image_layout(fmt, slice_type)
    if want_parity is None:
        want = list(range(m))
    else:
        want = sorted({int(r) for r in want_parity})
        if want and not 0 <= want[0] <= want[-1] < m:
            raise ValueError(f"want_parity: index out of [0, {m})")
    cols = view_columns(slice_type)
    ks = len(cols)
    shape, strides, addr = geom(data, "data", 3)
    if shape[0] != S or shape[1] < count.max() or shape[2] != size or \
            (size > 1 and strides[2] != 1) or \
            (shape[1] > 1 and strides[1] < size):
        raise ValueError(f"data must be [S={S}, >= {count.max()} blocks, "
                         f"{size}] with contiguous blocks")
    fragments = list(fragments)
    if len(fragments) != ks + m:
        raise ValueError(f"need {ks + m} fragment slots for slice type "
                         f"{slice_type}")
    if available is None:
        plans = [plan_write(slice_type, int(cb[s]), int(first[s]),
                            int(count[s])) for s in range(S)]
    else:
        plans = [plan_write_degraded(slice_type, available[s], int(cb[s]),
                                     int(first[s]), int(count[s]))
                 for s in range(S)]
        for s, plan in enumerate(plans):
            if plan is None:
                raise ValueError(f"chunk {s}: a fill column is lost and "
                                 f"fewer than {ks} parts are available")
    b = _Batch()
    b.S, b.ks, b.m, b.want, b.plans = S, ks, m, want, plans
    pars = _parity_parts(slice_type)
    b.wants = [want if available is None else
               [r for r in want if pars[r] in available[s]]
               for s in range(S)]
    b.slice_type, b.offset, b.size = slice_type, offset, size
    b.touched = np.array([len(p.rows) for p in plans], np.int64)
    b.count = count
    need = sorted({p for plan in plans for p in plan.read_parts})
    # the healthy call has a slot per view column, the degraded call a slot
    # per part that any write reads
    b.slots = list(cols) if available is None else (need or [cols[0]])
    if len(b.slots) > 32:
        raise ValueError(f"the writes read {len(b.slots)} parts; one call "
                         f"takes 32")
    b.fill = np.zeros((S, len(b.slots)), np.uint64)
    b.fill_nb = np.zeros((S, len(b.slots)), np.uint32)
    b.fill_stride = bstride
    b.first, b.chunk_blocks, b.available = first, cb, available
    for p in need:
        if fragments[p] is None:
            raise ValueError(f"fragment {p} is needed to fill the rows the "
                             f"writes touch in part")
        fshape, fstrides, faddr = geom(fragments[p], f"fragment {p}", 2)
        if fshape[0] != S or fstrides[1] != 1:
            raise ValueError(f"fragment {p} must be [S={S}, L] with "
                             f"contiguous rows")
        c = b.slots.index(p)
        for s in range(S):
            if p not in plans[s].read_parts:
                continue
            nb = _part_blocks(slice_type, p, int(cb[s]))
            if fshape[1] < data_off + (nb - 1) * bstride + _BLOCK:
                raise ValueError(f"fragment {p}: rows of {fshape[1]} bytes "
                                 f"cannot hold {nb} blocks")
            b.fill[s, c] = faddr + s * fstrides[0] + data_off
            b.fill_nb[s, c] = nb
    b.writes = np.zeros(S, WRITE_DTYPE)
    b.writes["data"] = addr + np.arange(S, dtype=np.uint64) * \
        np.uint64(strides[0])
    b.writes["data_stride"] = strides[1] if shape[1] > 1 else size
    b.writes["par_stride"] = m * size
    b.writes["first_block"] = first
    b.writes["block_count"] = count
    b.writes["from"] = offset
    b.writes["to"] = offset + size
    b.T = int(b.touched.max())
    b.ncrc = int(count.max()) + b.T * m
    return b


def _call(fn, head, b, par_addr, par_row_stride, crc_addr, crc_row_stride,
          tail):
    """par_addr / crc_addr: addresses of parity [S, T, m, size] and crcs
    [S, ncrc] with the given row strides."""
    u8p = ctypes.POINTER(ctypes.c_uint8)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    tbl = encode_table(b.slice_type)
    rows = np.arange(b.S, dtype=np.uint64)
    par = np.zeros((b.S, b.m), np.uint64)
    for r in b.want:
        par[:, r] = np.uint64(par_addr) + rows * np.uint64(par_row_stride) + \
            np.uint64(r * b.size)
    b.writes["crcs"] = np.uint64(crc_addr) + rows * np.uint64(crc_row_stride)
    return fn(*head, b.m, tbl.ctypes.data_as(u8p),
              ctypes.c_void_p(b.writes.ctypes.data), b.S,
              b.fill.ctypes.data_as(u64p), b.fill_nb.ctypes.data_as(u32p),
              b.ks, b.fill_stride, par.ctypes.data_as(u64p), *tail)


def _packets(b, data, parity, crcs):
    """crcs: host uint32 [S, ncrc].  Packets per chunk, in plan order."""
    cols = view_columns(b.slice_type)
    pars = _parity_parts(b.slice_type)
    out = []
    for s, plan in enumerate(b.plans):
        first, n = int(b.writes["first_block"][s]), int(b.count[s])
        r0 = first // b.ks
        pk = []
        for part, blk in plan.packets:
            if part in cols:
                i = blk * b.ks + cols.index(part) - first
                pk.append(Packet(part, blk, b.offset, b.size,
                                 int(crcs[s, i]), data[s, i]))
            else:
                r = pars.index(part)
                if r not in b.wants[s]:
                    continue
                pk.append(Packet(part, blk, b.offset, b.size,
                                 int(crcs[s, n + (blk - r0) * b.m + r]),
                                 parity[s, blk - r0, r]))
        out.append(pk)
    return out


def write_chunks(slice_type, fragments, chunk_blocks, data, first_block,
                 block_count, offset=0, size=_BLOCK, fmt=None,
                 want_parity=None):
    """Parity and packets of a batch of writes, one per chunk, into chunks
    held as an xor or ec slice, in one lizec_chunk_write_batch call.

    fragments: one slot per part of the slice; the slot of a data part that
      a write must read back (plan_write(...).read_parts) holds a [S, L]
      CUDA uint8 row view, the others may be None.  fmt = None: a row is the
      part's blocks back to back; "moosefs" / "interleaved": a row is a
      part-file image of that on-disk format (scrub.image_layout).
    chunk_blocks: S current chunk lengths in blocks, 0..1024.
    data: [S, B, size] CUDA uint8, data[s, i] the new bytes of chunk block
      first_block[s] + i; any alignment, any block stride >= size.
    first_block, block_count: one value each, or one per chunk; offset and
      size are the byte range inside every block, the same for the batch.
    want_parity: the parity indices (0..m-1) whose chunkservers are
      connected; None = all.
    The call runs on the device that holds `data`, on its current stream;
    the fragments that are read must lie on the same device.
    Returns (parity, crcs, packets): parity [S, T, m, size] uint8, T the
    most block rows a write touches, parity[s, i, r] parity r of the i-th
    row write s touches (unwanted or untouched entries are zeros); crcs
    [S, B' + T*m] int32 holding the CRCs' bit patterns as the library lays
    them out (lizec.h); packets[s] the Packets of write s in the
    reference's order, data packets viewing `data`.  Synchronises the
    stream to read the CRCs back.  Raises ValueError, before any GPU use,
    for what the library would refuse."""
    import torch

    def geom(t, what, dims):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or \
                not t.is_cuda or t.dim() != dims:
            raise ValueError(f"{what} must be a CUDA uint8 tensor of "
                             f"{dims} dimensions")
        return tuple(t.shape), tuple(t.stride()), t.data_ptr()

    def geom_on_device(t, what, dims):
        out = geom(t, what, dims)
        if t.device != data.device:
            raise ValueError(f"{what} lies on {t.device}, data on "
                             f"{data.device}")
        return out

    b = _prepare(slice_type, fragments, geom_on_device, chunk_blocks, data,
                 first_block, block_count, offset, size, fmt, want_parity)
    device = data.device.index
    parity = torch.zeros((b.S, b.T, b.m, size), dtype=torch.uint8,
                         device=data.device)
    crcs = torch.zeros((b.S, b.ncrc), dtype=torch.int32, device=data.device)
    stream = torch.cuda.current_stream(device)
    L.check(_call(L.lib().lizec_chunk_write_batch, (L.engine(device),), b,
                  parity.data_ptr(), parity.stride(0), crcs.data_ptr(),
                  4 * crcs.stride(0), (ctypes.c_void_p(stream.cuda_stream),)),
            "lizec_chunk_write_batch")
    stream.synchronize()
    host = crcs.cpu().numpy().view(np.uint32)
    return parity, crcs, _packets(b, data, parity, host)


def write_chunks_host(slice_type, fragments, chunk_blocks, data, first_block,
                      block_count, offset=0, size=_BLOCK, fmt=None,
                      want_parity=None):
    """write_chunks over numpy arrays, through lizec_chunk_write_host: no
    GPU is needed.  crcs comes back as uint32."""
    def geom(a, what, dims):
        if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or \
                a.ndim != dims:
            raise ValueError(f"{what} must be a uint8 array of {dims} "
                             f"dimensions")
        return a.shape, a.strides, a.ctypes.data

    b = _prepare(slice_type, fragments, geom, chunk_blocks, data, first_block,
                 block_count, offset, size, fmt, want_parity)
    parity = np.zeros((b.S, b.T, b.m, size), np.uint8)
    crcs = np.zeros((b.S, b.ncrc), np.uint32)
    L.check(_call(L.lib().lizec_chunk_write_host, (), b, parity.ctypes.data,
                  parity.strides[0], crcs.ctypes.data, crcs.strides[0], ()),
            "lizec_chunk_write_host")
    return parity, crcs, _packets(b, data, parity, crcs)


def _builder_part(slice_type, part):
    """A slice part in lizec_degraded_write_table's numbering: the data
    parts in column order, then the parity parts."""
    cols = view_columns(slice_type)
    if part in cols:
        return cols.index(part)
    return len(cols) + _parity_parts(slice_type).index(part)


def _degraded_tables(b):
    """The tables of a degraded batch, one per distinct (row shape,
    availability): (tables [n, m*(ks+srcs)*32], masks [n], index [S, 3])."""
    u8p = ctypes.POINTER(ctypes.c_uint8)
    t, ks, m, srcs = b.slice_type, b.ks, b.m, len(b.slots)
    cols = view_columns(t)
    slot_part = np.array([_builder_part(t, p) for p in b.slots], np.uint8)
    keys, tables, masks = {}, [], []
    index = np.zeros((b.S, 3), np.uint32)
    for s, plan in enumerate(b.plans):
        avail = sum(1 << _builder_part(t, p)
                    for p in _available(t, b.available[s], "available_parts"))
        nb = [_part_blocks(t, p, int(b.chunk_blocks[s])) for p in cols]
        shapes = [plan.rows[0], plan.rows[len(plan.rows) // 2],
                  plan.rows[-1]]
        for i, (row, kinds) in enumerate(shapes):
            new = sum(1 << c for c in range(ks) if kinds[c] == NEW)
            have = sum(1 << c for c in range(ks) if row < nb[c])
            key = (new, have, avail)
            if key not in keys:
                tbl = np.zeros(32 * (ks + srcs) * m, np.uint8)
                mask = ctypes.c_uint32()
                rc = L.lib().lizec_degraded_write_table(
                    ks, m, int(st.is_xor(t)), new, have, avail,
                    slot_part.ctypes.data_as(u8p), srcs,
                    tbl.ctypes.data_as(u8p), ctypes.byref(mask))
                if rc != 0:
                    # plan_write_degraded has found the chunk writable, so
                    # EINVAL here is a part the row needs without a slot
                    why = {-2: f"a part the row needs is not among the "
                               f"slots {b.slots} (plan and builder "
                               f"disagree)",
                           -1: "the surviving parts' matrix is singular"}
                    raise ValueError(
                        f"chunk {s}, row {row}: lizec_degraded_write_table "
                        f"{L._ERRNAMES.get(rc, rc)}: {why.get(rc, 'refused')}"
                        f"; new columns {new:#x}, columns with the row "
                        f"{have:#x}, available parts {avail:#x}")
                keys[key] = len(tables)
                tables.append(tbl)
                masks.append(mask.value)
            index[s, i] = keys[key]
    return np.stack(tables), np.array(masks, np.uint32), index


def _call_degraded(fn, head, b, tables, par_addr, par_row_stride, crc_addr,
                   crc_row_stride, tail):
    """_call for the degraded entry points."""
    u8p = ctypes.POINTER(ctypes.c_uint8)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    tbls, masks, index = tables
    rows = np.arange(b.S, dtype=np.uint64)
    par = np.zeros((b.S, b.m), np.uint64)
    for s in range(b.S):
        for r in b.wants[s]:
            par[s, r] = par_addr + s * par_row_stride + r * b.size
    b.writes["crcs"] = np.uint64(crc_addr) + rows * np.uint64(crc_row_stride)
    return fn(*head, b.m, tbls.ctypes.data_as(u8p), len(masks),
              masks.ctypes.data_as(u32p), index.ctypes.data_as(u32p),
              ctypes.c_void_p(b.writes.ctypes.data), b.S,
              b.fill.ctypes.data_as(u64p), b.fill_nb.ctypes.data_as(u32p),
              len(b.slots), b.ks, b.fill_stride, par.ctypes.data_as(u64p),
              *tail)


def _per_chunk_available(slice_type, available_parts, chunk_blocks):
    S = len(np.asarray(chunk_blocks).reshape(-1))
    av = list(available_parts)
    if all(isinstance(p, (int, np.integer)) for p in av):
        av = [av] * S
    if len(av) != S:
        raise ValueError(f"available_parts has {len(av)} entries for {S} "
                         f"chunks")
    _check_slice(slice_type, "slice_type")
    return [frozenset(_available(slice_type, a, "available_parts"))
            for a in av]


def write_chunks_degraded(slice_type, fragments, chunk_blocks, data,
                          first_block, block_count, available_parts,
                          offset=0, size=_BLOCK, fmt=None, want_parity=None):
    """write_chunks into chunks of which only available_parts (one set for
    the batch, or one per chunk) can be reached, in one
    lizec_chunk_write_degraded_batch call.

    fragments: as for write_chunks; the slots of the parts that a write
      reads (plan_write_degraded(...).read_parts: data parts and parity
      parts, as they are now) hold [S, L] CUDA uint8 row views.
    want_parity is intersected with every chunk's availability: a lost
      parity part is not computed and gets no packet, as a lost data part
      gets none for its new blocks.
    The parity comes back staged, never in place, so a parity part that is
    read as an old source is not overwritten by the call.
    Returns (parity, crcs, packets) like write_chunks.  Raises ValueError,
    before any GPU use, for what the library would refuse and for a chunk
    that cannot be written (a lost fill column with fewer than k parts
    available)."""
    import torch

    def geom(t, what, dims):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or \
                not t.is_cuda or t.dim() != dims:
            raise ValueError(f"{what} must be a CUDA uint8 tensor of "
                             f"{dims} dimensions")
        if isinstance(data, torch.Tensor) and t.device != data.device:
            raise ValueError(f"{what} lies on {t.device}, data on "
                             f"{data.device}")
        return tuple(t.shape), tuple(t.stride()), t.data_ptr()

    avail = _per_chunk_available(slice_type, available_parts, chunk_blocks)
    b = _prepare(slice_type, fragments, geom, chunk_blocks, data, first_block,
                 block_count, offset, size, fmt, want_parity, avail)
    tables = _degraded_tables(b)
    device = data.device.index
    parity = torch.zeros((b.S, b.T, b.m, size), dtype=torch.uint8,
                         device=data.device)
    crcs = torch.zeros((b.S, b.ncrc), dtype=torch.int32, device=data.device)
    stream = torch.cuda.current_stream(device)
    L.check(_call_degraded(L.lib().lizec_chunk_write_degraded_batch,
                           (L.engine(device),), b, tables, parity.data_ptr(),
                           parity.stride(0), crcs.data_ptr(),
                           4 * crcs.stride(0),
                           (ctypes.c_void_p(stream.cuda_stream),)),
            "lizec_chunk_write_degraded_batch")
    stream.synchronize()
    host = crcs.cpu().numpy().view(np.uint32)
    return parity, crcs, _packets(b, data, parity, host)


def write_chunks_degraded_host(slice_type, fragments, chunk_blocks, data,
                               first_block, block_count, available_parts,
                               offset=0, size=_BLOCK, fmt=None,
                               want_parity=None):
    """write_chunks_degraded over numpy arrays, through
    lizec_chunk_write_degraded_host: no GPU is needed.  crcs comes back as
    uint32."""
    def geom(a, what, dims):
        if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or \
                a.ndim != dims:
            raise ValueError(f"{what} must be a uint8 array of {dims} "
                             f"dimensions")
        return a.shape, a.strides, a.ctypes.data

    avail = _per_chunk_available(slice_type, available_parts, chunk_blocks)
    b = _prepare(slice_type, fragments, geom, chunk_blocks, data, first_block,
                 block_count, offset, size, fmt, want_parity, avail)
    tables = _degraded_tables(b)
    parity = np.zeros((b.S, b.T, b.m, size), np.uint8)
    crcs = np.zeros((b.S, b.ncrc), np.uint32)
    L.check(_call_degraded(L.lib().lizec_chunk_write_degraded_host, (), b,
                           tables, parity.ctypes.data, parity.strides[0],
                           crcs.ctypes.data, crcs.strides[0], ()),
            "lizec_chunk_write_degraded_host")
    return parity, crcs, _packets(b, data, parity, crcs)
