"""Chunkserver-side EC part rebuild — the compute core of
ChunkReplicator::replicate (chunk_replicator.cc:139-196), batched on GPU.

The reference's replicate loop pulls surviving parts from peers, recovers
the missing part via SliceRecoveryPlanner + ReedSolomon, CRCs every
recovered 64 KiB block (chunk_replicator.cc:189), and writes a MooseFS
part file.  Networking/disk stay with the host; this module does the whole
compute pipeline on the GPU: recover -> per-block CRC -> assembled part
image (header + big-endian CRC array + blocks) ready to pwrite.
"""
import collections
import ctypes

import numpy as np
import torch

from . import crc as lcrc
from . import lib as L
from . import scrub
from . import slice_traits as st
from .ec import ReedSolomon, _pattern_tables


def _rebuild_interleaved(rs, slice_type, fragments, erased, want, device):
    """rebuild_part_images for INTERLEAVED images: recover straight into
    the images' blocks (strided EC kernel), then fill the CRC slots."""
    doff, coff, bstride, cstride = scrub.image_layout("interleaved",
                                                      slice_type)
    surv = [f for i, f in enumerate(fragments)
            if f is not None and i not in set(erased)]
    if not surv:
        raise ValueError("all surviving parts are None")
    S, plen = surv[0].shape
    if plen % st.BLOCK_SIZE:
        raise ValueError("part length must be whole 64 KiB blocks")
    nblocks = plen // st.BLOCK_SIZE
    parts = sorted(set(want) if want is not None else set(erased))
    imgs = {p: torch.empty((S, nblocks * bstride), dtype=torch.uint8,
                           device=surv[0].device) for p in parts}
    rs.recover_batch_blocks(fragments, erased, want=parts,
                            out={p: imgs[p][:, doff:] for p in parts},
                            nblocks=nblocks, dst_stride=bstride)
    n = S * len(parts)
    dptrs = np.array([imgs[p].data_ptr() + s * nblocks * bstride
                      for p in parts for s in range(S)], np.uint64)
    doffs = np.full(n, doff, np.uint32)
    coffs = np.full(n, coff, np.uint32)
    counts = np.full(n, nblocks, np.uint32)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    stream = torch.cuda.current_stream(device).cuda_stream
    L.check(L.lib().lizec_crc_fill_batch_strided(
        L.engine(device), dptrs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
        doffs.ctypes.data_as(u32p), coffs.ctypes.data_as(u32p),
        counts.ctypes.data_as(u32p), n, bstride, cstride,
        ctypes.c_void_p(stream)), "lizec_crc_fill_batch_strided")
    return {(s, p): imgs[p][s] for p in parts for s in range(S)}


def _rebuild_ragged(rs, slice_type, fragments, erased, want, chunk_ids,
                    version, device, fmt, chunk_blocks):
    """rebuild_part_images for chunks of different lengths: every image has
    its own size; all of them are recovered in place by one ragged EC call
    and their CRCs filled by one call with per-image block counts."""
    doff, coff, bstride, cstride = scrub.image_layout(fmt, slice_type)
    nparts = rs.k + rs.m
    cb = np.asarray(chunk_blocks)
    if cb.ndim != 1 or cb.size < 1 or cb.dtype.kind not in "iu":
        raise ValueError("chunk_blocks must be a 1-D int sequence")
    if cb.min() < 1 or cb.max() > st.BLOCKS_IN_CHUNK:
        raise ValueError(f"chunk_blocks out of [1, {st.BLOCKS_IN_CHUNK}]")
    S = cb.size
    if fmt == "moosefs" and len(chunk_ids) != S:
        raise ValueError("need one chunk id per chunk")
    part_blocks = np.array(
        [[st.number_of_blocks(slice_type, i, int(n)) for i in range(nparts)]
         for n in cb], np.int64)
    S, dev, tables, index, slots, src, src_nb, dst_nb = rs._ragged_prepare(
        fragments, erased, want, part_blocks, st.BLOCK_SIZE,
        allow_empty=True)
    oc = slots.shape[1]
    # one arena; image (s, j) at offs[s, j], sized for its own block count
    used = slots >= 0
    head = doff if fmt == "moosefs" else 0
    sizes = np.where(used, head + dst_nb.astype(np.int64) *
                     (st.BLOCK_SIZE if fmt == "moosefs" else bstride), 0)
    offs = np.concatenate([[0], np.cumsum(sizes.ravel())[:-1]]).reshape(S, oc)
    arena = torch.empty(max(int(sizes.sum()), 1), dtype=torch.uint8,
                        device=dev)
    images = {}
    pairs = [(s, j) for s in range(S) for j in range(oc) if used[s, j]]
    for s, j in pairs:
        images[(s, int(slots[s, j]))] = \
            arena[int(offs[s, j]):int(offs[s, j] + sizes[s, j])]
    if fmt == "moosefs":
        # headers: zeros but for the signature; the CRC array is filled below
        hdrs = np.zeros((len(pairs), doff), np.uint8)
        for n, (s, j) in enumerate(pairs):
            sig = scrub.build_signature(int(chunk_ids[s]), version,
                                        slice_type, int(slots[s, j]))
            hdrs[n, :len(sig)] = np.frombuffer(sig, np.uint8)
        hdrs = torch.from_numpy(hdrs).to(dev)
        for n, (s, j) in enumerate(pairs):
            images[(s, int(slots[s, j]))][:doff] = hdrs[n]
    base = np.uint64(arena.data_ptr()) + offs.astype(np.uint64)
    fill = [(s, j) for s, j in pairs if dst_nb[s, j]]
    if fill:
        rs._ragged_call(tables, index, src, src_nb,
                        np.where(used, base + np.uint64(doff), np.uint64(0)),
                        dst_nb, st.BLOCK_SIZE, bstride)
        n = len(fill)
        dptrs = np.array([base[s, j] for s, j in fill], np.uint64)
        doffs = np.full(n, doff, np.uint32)
        coffs = np.full(n, coff, np.uint32)
        counts = np.array([dst_nb[s, j] for s, j in fill], np.uint32)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        stream = torch.cuda.current_stream(device).cuda_stream
        L.check(L.lib().lizec_crc_fill_batch_strided(
            L.engine(device),
            dptrs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
            doffs.ctypes.data_as(u32p), coffs.ctypes.data_as(u32p),
            counts.ctypes.data_as(u32p), n, bstride, cstride,
            ctypes.c_void_p(stream)), "lizec_crc_fill_batch_strided")
    return images


def rebuild_part_images(k, m, fragments, erased, want, chunk_ids, version,
                        device=0, fmt="moosefs", chunk_blocks=None):
    """Recover the `want` parts of a batch of chunks and build their part
    images on the GPU, in either on-disk format.

    fragments: list of k+m entries ([S, L] uint8 CUDA tensors or None),
      part data only (no headers), L a multiple of 64 KiB; row s belongs
      to chunk chunk_ids[s].
    erased: exactly m part indices (pad like ec_read_plan.h:126-133).
    want: subset of erased to rebuild.
    fmt: "moosefs" (default) or "interleaved" (no header or signature, each
      block preceded by its CRC; chunk_ids and version are unused there).
    chunk_blocks: optional, S block counts in 1..1024: chunk s is that many
      blocks long, so its part i has number_of_blocks(slice_type, i,
      chunk_blocks[s]) blocks (slice_traits.h:311-316) and the fragments
      are [S, Lmax] with rows read only that far.  Every returned image has
      its own chunk's size — header + nb*65536 (MooseFS), nb*65540
      (INTERLEAVED); a part of 0 blocks gives a header-only or empty image.
      erased / want may then also be per-stripe sets
      (ReedSolomon.recover_batch_ragged).
    Returns dict (chunk_index s, part_index) -> image tensor; image layout
    per chunkserver/chunk.cc (scrub.py geometry), CRC array filled by the
    GPU crc32_blocks kernel, signature per chunk_signature.cc:87-90.
    """
    slice_type = st.ec_slice_type(k, m)
    scrub.image_layout(fmt, slice_type)     # refuses an unknown fmt
    rs = ReedSolomon(k, m, device=device)
    if chunk_blocks is not None:
        return _rebuild_ragged(rs, slice_type, fragments, erased, want,
                               chunk_ids, version, device, fmt, chunk_blocks)
    if fmt == "interleaved":
        return _rebuild_interleaved(rs, slice_type, fragments, erased, want,
                                    device)
    rec = rs.recover_batch(fragments, erased=erased, want=want)

    out = {}
    hdr = scrub.header_size(slice_type)
    for part, data in rec.items():
        S, plen = data.shape
        if plen % st.BLOCK_SIZE:
            raise ValueError("part length must be whole 64 KiB blocks")
        nblocks = plen // st.BLOCK_SIZE
        # per-block CRCs for the whole batch at once, then byte-swap to the
        # on-disk big-endian layout (put32bit convention)
        crcs = lcrc.crc32_blocks(data.reshape(-1), st.BLOCK_SIZE)
        be = crcs.view(torch.uint8).reshape(S, nblocks, 4).flip(dims=(2,))
        for s in range(S):
            img = torch.zeros(hdr + plen, dtype=torch.uint8,
                              device=data.device)
            sig = scrub.build_signature(int(chunk_ids[s]), version,
                                        slice_type, part)
            img[:len(sig)] = torch.from_numpy(
                np.frombuffer(sig, np.uint8).copy()).to(data.device)
            img[scrub.SIGNATURE_BLOCK:
                scrub.SIGNATURE_BLOCK + 4 * nblocks] = be[s].reshape(-1)
            img[hdr:] = data[s]
            out[(s, part)] = img
    return out


def convert_part_images(src_slice, fragments, chunk_blocks, target_slice,
                        want, chunk_ids, version, fmt="moosefs",
                        src_erased=None, src_stride=st.BLOCK_SIZE, device=0):
    """convert.convert_parts straight into part images: the `want` parts of
    `target_slice` for chunks held as `src_slice` (a goal change), each image
    in on-disk format `fmt` and sized for its own chunk, recovered in place
    by the view calls and its CRCs filled by lizec_crc_fill_batch_strided,
    exactly as rebuild_part_images(chunk_blocks=...) does for a rebuild from
    the part's own slice.

    src_slice, fragments, chunk_blocks, target_slice, want, src_erased,
    src_stride: as for convert_parts.  chunk_ids, version, fmt: as for
    rebuild_part_images.
    Returns dict (chunk_index s, target part) -> image tensor.
    """
    from . import convert
    doff, coff, bstride, cstride = scrub.image_layout(fmt, target_slice)
    plan = convert._prepare(src_slice, fragments, chunk_blocks, target_slice,
                            want, src_erased, src_stride, device)
    S, oc = plan.slots.shape
    if fmt == "moosefs" and len(chunk_ids) != S:
        raise ValueError("need one chunk id per chunk")
    slots, dst_nb, dev = plan.slots, plan.dst_nb, plan.dev
    # one arena; image (s, j) at offs[s, j], sized for its own block count
    used = slots >= 0
    head = doff if fmt == "moosefs" else 0
    sizes = np.where(used, head + dst_nb.astype(np.int64) *
                     (st.BLOCK_SIZE if fmt == "moosefs" else bstride), 0)
    offs = np.concatenate([[0], np.cumsum(sizes.ravel())[:-1]]).reshape(S, oc)
    arena = torch.empty(max(int(sizes.sum()), 1), dtype=torch.uint8,
                        device=dev)
    images = {}
    pairs = [(s, j) for s in range(S) for j in range(oc) if used[s, j]]
    for s, j in pairs:
        images[(s, int(slots[s, j]))] = \
            arena[int(offs[s, j]):int(offs[s, j] + sizes[s, j])]
    if fmt == "moosefs":
        hdrs = np.zeros((len(pairs), doff), np.uint8)
        for n, (s, j) in enumerate(pairs):
            sig = scrub.build_signature(int(chunk_ids[s]), version,
                                        target_slice, int(slots[s, j]))
            hdrs[n, :len(sig)] = np.frombuffer(sig, np.uint8)
        hdrs = torch.from_numpy(hdrs).to(dev)
        for n, (s, j) in enumerate(pairs):
            images[(s, int(slots[s, j]))][:doff] = hdrs[n]
    base = np.uint64(arena.data_ptr()) + offs.astype(np.uint64)
    fill = [(s, j) for s, j in pairs if dst_nb[s, j]]
    if fill:
        plan.run(base + np.uint64(doff), bstride)
        n = len(fill)
        dptrs = np.array([base[s, j] for s, j in fill], np.uint64)
        doffs = np.full(n, doff, np.uint32)
        coffs = np.full(n, coff, np.uint32)
        counts = np.array([dst_nb[s, j] for s, j in fill], np.uint32)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        stream = torch.cuda.current_stream(device).cuda_stream
        L.check(L.lib().lizec_crc_fill_batch_strided(
            L.engine(device),
            dptrs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
            doffs.ctypes.data_as(u32p), coffs.ctypes.data_as(u32p),
            counts.ctypes.data_as(u32p), n, bstride, cstride,
            ctypes.c_void_p(stream)), "lizec_crc_fill_batch_strided")
    return images


def _check_rows(a, what):
    """The C side is handed one address per row (base + s*strides[0]) and
    takes a row's bytes to be contiguous there: rows may lie any distance
    apart, but not backwards (the address arithmetic is unsigned), and a
    row's bytes must be adjacent."""
    if a.strides[1] != 1:
        raise ValueError(f"{what}: rows must be contiguous "
                         f"(inner stride {a.strides[1]}, not 1)")
    if a.strides[0] < 0:
        raise ValueError(f"{what}: negative row stride {a.strides[0]}")


def replicate_stream(k, m, host_parts, erased, want, chunk_ids, version,
                     out=None, device=0, sub_batch=0, fmt="moosefs"):
    """The full ChunkReplicator::replicate pipeline
    (chunk_replicator.cc:139-196), host-to-host and streaming: surviving
    parts in HOST memory -> H2D -> recover -> per-block CRC -> MooseFS part
    image assembly on-device -> D2H, double-buffered (lizec_replicate_run).

    host_parts: list of k+m entries; entry i is a numpy uint8 [S, L] array
      (surviving part bytes, L a multiple of 64 KiB) or None (erased).
      Use lib.pinned_empty for true copy/compute overlap.  Rows may lie any
      distance apart (a row-strided view is fine), but each row's bytes
      must be contiguous and the row stride not negative; the same holds
      for the arrays of `out`.  Anything else raises ValueError.
    erased: exactly m part indices; want: subset to rebuild.
    out: optional dict part -> uint8 [S, hdr+L] array to fill (pinned
      recommended); allocated (pinned) if absent.
    fmt: "moosefs" (default) or "interleaved"
      (lizec_replicate_run_interleaved): images of (L/65536)*65540 bytes,
      no header or signature, each block preceded by its big-endian CRC;
      chunk_ids and version are unused there.
    Returns dict part -> [S, hdr+L] images (signature + BE CRC array +
    recovered blocks), pwrite-ready.
    """
    if fmt not in scrub.FORMATS:
        raise ValueError(f"unknown chunk format {fmt!r} "
                         f"(one of {scrub.FORMATS})")
    nparts = k + m
    if len(host_parts) != nparts:
        raise ValueError(f"need {nparts} part slots")
    erased = sorted(set(erased))
    if len(erased) != m:
        raise ValueError(f"exactly m={m} erased parts required")
    want = sorted(set(want)) if want is not None else erased
    if not set(want).issubset(erased):
        raise ValueError("want must be a subset of erased")
    surv = [i for i in range(nparts) if i not in erased]
    S = plen = None
    for i in surv:
        if host_parts[i] is None:
            raise ValueError(f"surviving part {i} is None (streaming path "
                             f"takes explicit zero buffers)")
        a = host_parts[i]
        if a.dtype != np.uint8 or a.ndim != 2:
            raise ValueError("parts must be uint8 [S, L]")
        if S is None:
            S, plen = a.shape
        elif a.shape != (S, plen):
            raise ValueError("part shapes differ")
        _check_rows(a, f"part {i}")
    if plen % st.BLOCK_SIZE:
        raise ValueError("part length must be whole 64 KiB blocks")
    if len(chunk_ids) != S:
        raise ValueError("need one chunk id per stripe")

    slice_type = st.ec_slice_type(k, m)
    hdr = scrub.header_size(slice_type)
    img_bytes = hdr + plen
    if fmt == "interleaved":
        img_bytes = plen // st.BLOCK_SIZE * scrub.HDD_BLOCK
    if out is not None:
        for p in want:
            if p not in out:
                raise ValueError(f"out has no array for wanted part {p}")
            a = out[p]
            if a.dtype != np.uint8 or a.shape != (S, img_bytes):
                raise ValueError(
                    f"out[{p}] must be uint8 [S={S}, {img_bytes}]")
            _check_rows(a, f"out[{p}]")
            if S > 1 and a.strides[0] < img_bytes:
                raise ValueError(f"out[{p}]: rows overlap (row stride "
                                 f"{a.strides[0]} < {img_bytes})")
    present = sum(1 << i for i in surv)
    needed = sum(1 << i for i in want)
    lib = L.lib()
    tbl = np.zeros(32 * 32 * 32, np.uint8)
    ic = ctypes.c_int()
    oc = ctypes.c_int()
    L.check(lib.lizec_rs_tables(
        k, m, present, present, needed,
        tbl.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
        ctypes.byref(ic), ctypes.byref(oc)), "lizec_rs_tables")
    ic, oc = ic.value, oc.value
    assert (ic, oc) == (len(surv), len(want))

    if out is None:
        out = {p: L.pinned_empty((S, img_bytes)) for p in want}

    src = np.empty((S, ic), np.uint64)
    for j, i in enumerate(surv):
        a = host_parts[i]
        src[:, j] = a.ctypes.data + np.arange(S, dtype=np.uint64) * \
            np.uint64(a.strides[0])
    dst = np.empty((S, oc), np.uint64)
    sigs = np.zeros((S, oc, 22), np.uint8)
    for j, p in enumerate(want):
        a = out[p]
        dst[:, j] = a.ctypes.data + np.arange(S, dtype=np.uint64) * \
            np.uint64(a.strides[0])
        for s in range(S if fmt == "moosefs" else 0):
            sig = scrub.build_signature(int(chunk_ids[s]), version,
                                        slice_type, p)
            sigs[s, j, :len(sig)] = np.frombuffer(sig, np.uint8)

    if fmt == "interleaved":
        L.check(lib.lizec_replicate_run_interleaved(
            L.engine(device), plen, ic, oc,
            tbl.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
            np.ascontiguousarray(src.ravel()).ctypes.data_as(
                ctypes.POINTER(ctypes.c_uint64)),
            np.ascontiguousarray(dst.ravel()).ctypes.data_as(
                ctypes.POINTER(ctypes.c_uint64)),
            S, sub_batch), "lizec_replicate_run_interleaved")
        return out
    L.check(lib.lizec_replicate_run(
        L.engine(device), plen, ic, oc,
        tbl.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
        np.ascontiguousarray(src.ravel()).ctypes.data_as(
            ctypes.POINTER(ctypes.c_uint64)),
        sigs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
        22, hdr, scrub.SIGNATURE_BLOCK,
        np.ascontiguousarray(dst.ravel()).ctypes.data_as(
            ctypes.POINTER(ctypes.c_uint64)),
        S, sub_batch), "lizec_replicate_run")
    return out


StreamRebuild = collections.namedtuple("StreamRebuild", "images corrupt")
StreamRebuild.__doc__ = """Result of replicate_stream_ragged: `images` maps
(chunk index, part) to the part's image, `corrupt` maps a chunk index to the
set of source parts that failed their CRC check (such chunks have no entry in
`images`)."""

REPL_INTERLEAVED = 1        # LIZEC_REPL_INTERLEAVED


def _stream_ragged_prepare(k, m, host_parts, chunk_blocks, erased, want,
                           chunk_ids, version, crcs, out, fmt):
    """Every argument check of replicate_stream_ragged and the host arrays of
    the C call; touches neither an engine nor the GPU."""
    slice_type = st.ec_slice_type(k, m)
    doff, coff, bstride, cstride = scrub.image_layout(fmt, slice_type)
    nparts = k + m
    if len(host_parts) != nparts:
        raise ValueError(f"need {nparts} part slots")
    cb = np.asarray(chunk_blocks)
    if cb.ndim != 1 or cb.size < 1 or cb.dtype.kind not in "iu":
        raise ValueError("chunk_blocks must be a 1-D int sequence")
    if cb.min() < 1 or cb.max() > st.BLOCKS_IN_CHUNK:
        raise ValueError(f"chunk_blocks out of [1, {st.BLOCKS_IN_CHUNK}]")
    S = cb.size
    if fmt == "moosefs" and len(chunk_ids) != S:
        raise ValueError("need one chunk id per chunk")
    pb = np.array([[st.number_of_blocks(slice_type, i, int(n))
                    for i in range(nparts)] for n in cb], np.int64)
    erased = ReedSolomon._per_stripe_sets(None, erased, S, "erased")
    if want is not None:
        want = ReedSolomon._per_stripe_sets(None, want, S, "want")
    tables, index, pslots, pemask = _pattern_tables(k, m, erased, want)
    slots = pslots[index]                                      # [S, oc]
    oc = slots.shape[1]
    palive = np.array([[i for i in range(nparts) if not (int(e) >> i) & 1]
                       for e in pemask], np.intp)
    alive = palive[index]                                      # [S, k]
    src_nb = np.ascontiguousarray(
        np.take_along_axis(pb, alive, axis=1).astype(np.uint32))
    # blocks that are read of part i: the longest count among the chunks in
    # which it survives
    top = np.zeros(nparts, np.int64)
    np.maximum.at(top, alive.ravel(), src_nb.ravel().astype(np.int64))
    survives = np.zeros(nparts, bool)
    survives[np.unique(alive)] = True
    if crcs is not None and len(crcs) != nparts:
        raise ValueError(f"crcs needs {nparts} part slots")
    bases = np.zeros(nparts, np.uint64)
    strides = np.zeros(nparts, np.uint64)
    cbases = np.zeros(nparts, np.uint64)
    cstrides = np.zeros(nparts, np.uint64)
    for i in range(nparts):
        if not survives[i]:
            continue
        a = host_parts[i]
        if a is None:
            raise ValueError(f"part {i} is None but survives in some chunk")
        if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or \
                a.ndim != 2:
            raise ValueError(f"part {i} must be a numpy uint8 [S, Lmax] array")
        if a.shape[0] != S:
            raise ValueError(f"part {i} has {a.shape[0]} rows, expected {S}")
        _check_rows(a, f"part {i}")
        if a.shape[1] < top[i] * st.BLOCK_SIZE:
            raise ValueError(f"part {i}: rows of {a.shape[1]} bytes cannot "
                             f"hold {int(top[i])} blocks")
        bases[i] = a.ctypes.data
        strides[i] = a.strides[0]
        c = crcs[i] if crcs is not None else None
        if c is None:
            continue
        if not isinstance(c, np.ndarray) or c.shape[0] != S or not (
                (c.ndim == 2 and c.dtype == np.dtype(">u4")) or
                (c.ndim == 3 and c.dtype == np.uint8 and c.shape[2] == 4)):
            raise ValueError(f"crcs[{i}] must be [S, nmax] big-endian '>u4' "
                             f"or [S, nmax, 4] uint8")
        if c.shape[1] < top[i]:
            raise ValueError(f"crcs[{i}]: rows of {c.shape[1]} CRCs cannot "
                             f"cover {int(top[i])} blocks")
        if c.strides[0] < 0 or (c.shape[1] > 1 and c.strides[1] != 4) or \
                (c.ndim == 3 and c.strides[2] != 1):
            raise ValueError(f"crcs[{i}]: a row's CRCs must be contiguous, "
                             f"4 bytes apart, and the row stride not "
                             f"negative")
        cbases[i] = c.ctypes.data
        cstrides[i] = c.strides[0]
    rows = np.arange(S, dtype=np.uint64)[:, None]
    src = np.where(src_nb > 0, bases[alive] + rows * strides[alive],
                   np.uint64(0)).astype(np.uint64)
    src_crc = None
    if crcs is not None:
        src_crc = np.where(cbases[alive] != 0,
                           cbases[alive] + rows * cstrides[alive],
                           np.uint64(0)).astype(np.uint64)
    used = slots >= 0
    dst_nb = np.take_along_axis(pb, np.maximum(slots, 0), axis=1)
    dst_nb = np.ascontiguousarray(np.where(used, dst_nb, 0).astype(np.uint32))
    head = doff if fmt == "moosefs" else 0
    sizes = np.where(used, head + dst_nb.astype(np.int64) *
                     (st.BLOCK_SIZE if fmt == "moosefs" else bstride), 0)
    pairs = [(s, j) for s in range(S) for j in range(oc) if used[s, j]]
    if out is not None:
        for s, j in pairs:
            key = (s, int(slots[s, j]))
            if key not in out:
                raise ValueError(f"out has no array for wanted image {key}")
            a = out[key]
            if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or \
                    a.ndim != 1 or a.shape[0] != sizes[s, j]:
                raise ValueError(f"out[{key}] must be a 1-D uint8 array of "
                                 f"{int(sizes[s, j])} bytes")
            if a.shape[0] > 1 and a.strides[0] != 1:
                raise ValueError(f"out[{key}] must be contiguous")
    sigs = np.zeros((S, oc, 22), np.uint8)
    if fmt == "moosefs":
        for s, j in pairs:
            sig = scrub.build_signature(int(chunk_ids[s]), version,
                                        slice_type, int(slots[s, j]))
            sigs[s, j, :len(sig)] = np.frombuffer(sig, np.uint8)
    return dict(S=S, oc=oc, tables=tables, index=index, slots=slots,
                alive=alive, src=np.ascontiguousarray(src), src_nb=src_nb,
                src_crc=src_crc, dst_nb=dst_nb, sizes=sizes, pairs=pairs,
                sigs=sigs, head=head, coff=coff,
                flags=REPL_INTERLEAVED if fmt == "interleaved" else 0)


def _stream_ragged_run(k, p, out, alloc, call):
    """Lay the images out (the caller's arrays, or one arena from `alloc`),
    make the C call through `call` and sort its results."""
    S, oc, slots, sizes = p["S"], p["oc"], p["slots"], p["sizes"]
    dst = np.zeros((S, oc), np.uint64)
    images = {}
    if out is None:
        # every image 16-aligned in one arena
        offs = np.concatenate([[0], np.cumsum((sizes.ravel() + 15) & ~15)])
        arena = alloc(max(int(offs[-1]), 1))
        offs = offs[:-1].reshape(S, oc)
        for s, j in p["pairs"]:
            a = arena[int(offs[s, j]):int(offs[s, j] + sizes[s, j])]
            images[(s, int(slots[s, j]))] = a
            dst[s, j] = arena.ctypes.data + int(offs[s, j])
    else:
        for s, j in p["pairs"]:
            a = out[(s, int(slots[s, j]))]
            images[(s, int(slots[s, j]))] = a
            # an empty INTERLEAVED image is nothing at all: not wanted
            dst[s, j] = a.ctypes.data if a.shape[0] else 0
    bad = np.zeros(S, np.uint32)
    u8p = ctypes.POINTER(ctypes.c_uint8)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    verify = p["src_crc"] is not None
    src_crc = np.ascontiguousarray(p["src_crc"]) if verify else None
    call(k, oc, p["tables"].ctypes.data_as(u8p), p["tables"].shape[0],
         p["index"].ctypes.data_as(u32p), p["src"].ctypes.data_as(u64p),
         p["src_nb"].ctypes.data_as(u32p),
         src_crc.ctypes.data_as(u64p) if verify else None,
         p["sigs"].ctypes.data_as(u8p), 22, p["head"], p["coff"],
         dst.ctypes.data_as(u64p), p["dst_nb"].ctypes.data_as(u32p), S,
         p["flags"], bad.ctypes.data_as(u32p) if verify else None)
    corrupt = {}
    for s in np.flatnonzero(bad):
        s = int(s)
        corrupt[s] = {int(p["alive"][s, j]) for j in range(k)
                      if (int(bad[s]) >> j) & 1}
        for j in range(oc):
            images.pop((s, int(slots[s, j])), None)
    return StreamRebuild(images, corrupt)


def replicate_stream_ragged(k, m, host_parts, chunk_blocks, erased, want,
                            chunk_ids, version, crcs=None, out=None, device=0,
                            stage_bytes=0, fmt="moosefs"):
    """replicate_stream for chunks of any length and erasure pattern, with
    the sources verified on the way through (lizec_replicate_run_ragged):
    surviving parts in HOST memory -> H2D -> CRC check -> recover -> per-block
    CRC -> image assembly on-device -> D2H, double-buffered.

    host_parts: k+m entries, numpy uint8 [S, Lmax] or None; row s of part i
      is read only up to number_of_blocks(slice_type, i, chunk_blocks[s])
      blocks.  Rows as for replicate_stream.  None only for a part that is
      erased in every chunk.
    chunk_blocks: S block counts in 1..1024.
    erased / want: one index set for all chunks, or one per chunk (exactly m
      erased each, want a subset), as for ReedSolomon.recover_batch_ragged.
    crcs: optional list like host_parts of [S, nmax] big-endian '>u4' or
      [S, nmax, 4] uint8 arrays: the CRC of every block of the part, as a
      MooseFS part file holds them at offset 1024.  None = that part is not
      verified.
    out: optional dict (s, part) -> 1-D uint8 array of exactly the image's
      size; otherwise the images are views into one pinned arena.
    stage_bytes: device staging per pipeline slot (0 = 2 GiB).
    fmt: "moosefs" or "interleaved"; chunk_ids and version are unused in the
      latter.
    Returns StreamRebuild(images, corrupt): images maps (s, part) to the
    pwrite-ready image of that chunk's own size (header + nb*65536, or
    nb*65540); corrupt maps s to the set of parts whose CRC check failed,
    and those chunks are left out of images.
    """
    p = _stream_ragged_prepare(k, m, host_parts, chunk_blocks, erased, want,
                               chunk_ids, version, crcs, out, fmt)
    if not 0 <= stage_bytes <= 1 << 31:
        raise ValueError("stage_bytes out of [0, 2^31]")
    eng = L.engine(device)

    def call(*a):
        L.check(L.lib().lizec_replicate_run_ragged(
            eng, *a[:-2], stage_bytes, *a[-2:]), "lizec_replicate_run_ragged")
    return _stream_ragged_run(k, p, out, L.pinned_empty, call)


def replicate_stream_ragged_host(k, m, host_parts, chunk_blocks, erased, want,
                                 chunk_ids, version, crcs=None, out=None,
                                 device=0, stage_bytes=0, fmt="moosefs"):
    """replicate_stream_ragged on the CPU (lizec_replicate_ragged_host): same
    arguments (device and stage_bytes are unused) and the same result byte
    for byte; needs no GPU."""
    p = _stream_ragged_prepare(k, m, host_parts, chunk_blocks, erased, want,
                               chunk_ids, version, crcs, out, fmt)

    def call(*a):
        L.check(L.lib().lizec_replicate_ragged_host(*a),
                "lizec_replicate_ragged_host")
    return _stream_ragged_run(k, p, out, lambda n: np.empty(n, np.uint8),
                              call)
