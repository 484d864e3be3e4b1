"""Parts of one slice type built from a chunk held in another — the goal
change path (2 copies -> ec(8,2), ec(3,2) -> ec(8,2), ...), batched on GPU.

SliceRecoveryPlanner (slice_recovery_planner.h:85-204) builds a part in one
of three ways: it reads it from its own slice (kReadDataPart, what
ReedSolomon.recover_batch* serve), or it reads the chunk's data from a slice
of another type as consecutive blocks (chunk_read_planner.h:36-58) and then
either cuts a data part out of them at stride k (kRecoverDataPart, :41-55)
or computes a parity part over rows of k consecutive blocks
(kRecoverParityPart, ec_read_plan.h:38-66, xor_read_plan.h:39).  The last
two are lizec_ec_encode_batch_view: the kernel walks the source slice's data
parts round-robin, so the chunk is never assembled.
"""
import ctypes

import numpy as np
import torch

from . import lib as L
from . import slice_traits as st
from .ec import ReedSolomon, _pattern_table

_BLOCK = st.BLOCK_SIZE


def _check_slice(t, what):
    if not (t == st.K_STANDARD or st.is_xor(t) or st.is_ec(t)):
        raise ValueError(f"{what}: slice type {t} is neither standard, xor "
                         f"nor ec")


def _total_parts(t):
    return st.data_parts(t) + st.parity_parts(t)


def _data_index(t, part):
    """Data index of a slice part, None for a parity part.  A xor slice
    keeps its parity at part 0 (slice_traits.h:98, 283-288)."""
    if st.is_xor(t):
        return part - 1 if part >= 1 else None
    return part if part < st.data_parts(t) else None


def _part_blocks(t, part, n):
    """Blocks of a part of a chunk of n blocks (slice_traits.h:311-316); a
    parity part is as long as data part 0."""
    d = _data_index(t, part)
    # number_of_blocks takes a data part by its index and anything from
    # data_parts on as a parity part
    return st.number_of_blocks(t, st.data_parts(t) if d is None else d, n)


def view_columns(slice_type):
    """View column -> slice part: the data parts of a slice in the order in
    which consecutive chunk blocks walk through them."""
    _check_slice(slice_type, "view_columns")
    k = st.data_parts(slice_type)
    if st.is_xor(slice_type):
        return list(range(1, k + 1))
    return list(range(k))


def chunk_block_range(target_slice, target_part, first_block, block_count):
    """(first chunk block, count) that SliceRecoveryPlanner::prepare asks
    of the chunk planner for blocks [first_block, first_block + block_count)
    of a part (slice_recovery_planner.h:99-115)."""
    k = st.data_parts(target_slice)
    d = _data_index(target_slice, target_part)
    if d is not None:
        return d + first_block * k, 1 + (block_count - 1) * k
    return first_block * k, block_count * k


def _slice_readable(slice_type, parts, available):
    """SliceReadPlanner::isReadingPossible (slice_read_planner.cc:46-51)."""
    have = {p for t, p in available if t == slice_type}
    return all(p in have for p in parts) or \
        len(have) >= st.data_parts(slice_type)


def _required_parts(slice_type, first_block, block_count):
    """ChunkReadPlanner::getRequiredParts (chunk_read_planner.h:182-206)."""
    cols = view_columns(slice_type)
    k = len(cols)
    if block_count >= k:
        return cols
    return [cols[(first_block + i) % k] for i in range(block_count)]


def recovery_method(target_slice, target_part, available, first_block=0,
                    block_count=None):
    """How SliceRecoveryPlanner::prepare would build blocks [first_block,
    first_block + block_count) of a part (default: the part of a full
    chunk), in its order of choice:
      "read"   — from the part's own slice (kReadDataPart);
      "data"   — a data part cut from the chunk read from another slice;
      "parity" — a parity part computed over the chunk read likewise;
      None     — nothing readable.
    available: (slice_type, part) pairs.  The chunk blocks the two chunk
    methods read are chunk_block_range(...).  Pure Python."""
    _check_slice(target_slice, "target_slice")
    if not 0 <= target_part < _total_parts(target_slice):
        raise ValueError(f"part {target_part} outside slice {target_slice}")
    available = [(int(t), int(p)) for t, p in available]
    if block_count is None:
        block_count = _part_blocks(target_slice, target_part,
                                   st.BLOCKS_IN_CHUNK) - first_block
    if first_block < 0 or block_count < 1:
        raise ValueError("empty block range")
    if _slice_readable(target_slice, [target_part], available):
        return "read"
    first, count = chunk_block_range(target_slice, target_part, first_block,
                                     block_count)
    types = []
    for t, _ in available:              # getTypeList: first-seen order
        if t not in types:
            types.append(t)
    for t in types:
        if t != st.K_STANDARD and not st.is_xor(t) and not st.is_ec(t):
            continue
        if _slice_readable(t, _required_parts(t, first, count), available):
            return "data" if _data_index(target_slice, target_part) \
                is not None else "parity"
    return None


def _want_sets(want, S, nparts):
    sets = list(want)
    if all(isinstance(i, (int, np.integer)) for i in sets):
        sets = [sets] * S
    if len(sets) != S:
        raise ValueError(f"want has {len(sets)} entries for {S} chunks")
    out = []
    for s, w in enumerate(sets):
        w = sorted({int(i) for i in w})
        if w and not 0 <= w[0] <= w[-1] < nparts:
            raise ValueError(f"want[{s}]: part index out of [0, {nparts})")
        out.append(w)
    if not any(out):
        raise ValueError("no part is wanted")
    return out


def _frag_geom(t, what):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or \
            not t.is_cuda or t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{what} must be a CUDA uint8 [S, L] tensor with "
                         f"contiguous rows")
    return t.shape[0], t.shape[1], t.stride(0)


class _Plan:
    """A checked conversion: who gets what (slots, dst_nb) and the two view
    calls that produce it, run(dst [S, oc] addresses, dst_stride)."""


def _prepare(src_slice, fragments, chunk_blocks, target_slice, want,
             src_erased, src_stride, device):
    _check_slice(src_slice, "src_slice")
    _check_slice(target_slice, "target_slice")
    cb = np.asarray(chunk_blocks)
    if cb.ndim != 1 or cb.size < 1 or cb.dtype.kind not in "iu":
        raise ValueError("chunk_blocks must be a 1-D int sequence")
    if cb.min() < 1 or cb.max() > st.BLOCKS_IN_CHUNK:
        raise ValueError(f"chunk_blocks out of [1, {st.BLOCKS_IN_CHUNK}]")
    S = cb.size
    if src_stride < _BLOCK or src_stride % 4:
        raise ValueError(f"src_stride={src_stride} must be a multiple of 4 "
                         f"and at least {_BLOCK}")
    nsrc = _total_parts(src_slice)
    fragments = list(fragments)
    if len(fragments) != nsrc:
        raise ValueError(f"need {nsrc} fragment slots for slice type "
                         f"{src_slice}")
    ntgt = _total_parts(target_slice)
    wants = _want_sets(want, S, ntgt)
    cols = view_columns(src_slice)
    ks, kt = len(cols), st.data_parts(target_slice)
    erased = None
    if src_erased is not None:
        if not st.is_ec(src_slice):
            raise ValueError("src_erased needs an ec source: a degraded "
                             "xor or standard source is not converted")
        erased = list(src_erased)
        if erased and all(isinstance(i, (int, np.integer)) for i in erased):
            erased = [erased] * S
        if len(erased) != S:
            raise ValueError(f"src_erased has {len(erased)} entries for "
                             f"{S} chunks")
        m = st.parity_parts(src_slice)
        padded = []
        for s, e in enumerate(erased):
            e = sorted({int(i) for i in e})
            if e and not 0 <= e[0] <= e[-1] < nsrc:
                raise ValueError(f"src_erased[{s}]: part index out of "
                                 f"[0, {nsrc})")
            if len(e) > m:
                raise ValueError(f"src_erased[{s}]: more than m={m} parts")
            # pad to exactly m with the highest parts (ec_read_plan.h:126-133)
            pad = [i for i in range(nsrc - 1, -1, -1) if i not in e]
            padded.append(sorted(e + pad[:m - len(e)]))
            for p in range(nsrc):
                if p not in padded[-1] and fragments[p] is None:
                    raise ValueError(f"fragment {p} is None but survives in "
                                     f"chunk {s}")
        erased = padded
    # the view columns each chunk uses, and who provides them
    used = np.arange(ks)[None, :] < cb[:, None]                   # [S, ks]
    lost = np.zeros((S, ks), bool)
    if erased is not None:
        for s, e in enumerate(erased):
            lost[s, [c for c in range(ks) if cols[c] in e]] = True
    for c, p in enumerate(cols):
        if fragments[p] is None and (used[:, c] & ~lost[:, c]).any():
            if st.is_xor(src_slice):
                raise ValueError(f"fragment {p} is None: a degraded xor "
                                 f"source is not converted")
            raise ValueError(f"fragment {p} is None but holds blocks of a "
                             f"chunk")
    src_nb = np.array([[_part_blocks(src_slice, p, int(n))
                        for p in range(nsrc)] for n in cb], np.int64)
    bases = np.zeros(nsrc, np.uint64)
    strides = np.zeros(nsrc, np.uint64)
    dev = None
    for p, t in enumerate(fragments):
        if t is None:
            continue
        s, span, rstride = _frag_geom(t, f"fragment {p}")
        if s != S:
            raise ValueError(f"fragment {p} has {s} rows, expected {S}")
        top = int(src_nb[:, p].max())
        need = (top - 1) * src_stride + _BLOCK if top else 0
        if span < need:
            raise ValueError(f"fragment {p}: rows of {span} bytes cannot "
                             f"hold {top} blocks at stride {src_stride} "
                             f"({need} bytes)")
        if t.data_ptr() % 4 or (s > 1 and rstride % 4):
            raise ValueError(f"fragment {p}: block data must be 4-byte "
                             f"aligned")
        dev = t.device
        bases[p], strides[p] = t.data_ptr(), rstride
    if dev is None:
        raise ValueError("all fragments are None")

    plan = _Plan()
    plan.S, plan.dev, plan.device = S, dev, device
    oc = max(len(w) for w in wants)
    plan.slots = np.full((S, oc), -1, np.int64)
    plan.dst_nb = np.zeros((S, oc), np.uint32)
    for s, w in enumerate(wants):
        plan.slots[s, :len(w)] = w
        plan.dst_nb[s, :len(w)] = [_part_blocks(target_slice, p, int(cb[s]))
                                   for p in w]

    def run(dst, dst_stride):
        rows = np.arange(S, dtype=np.uint64)[:, None]
        view = bases[cols][None, :] + rows * strides[cols][None, :]
        keep = None
        if erased is not None and (lost & used).any():
            # rebuild the lost data parts of the source slice first; the
            # view then points at the rebuilt copies
            rs = ReedSolomon(ks, st.parity_parts(src_slice), device=device)
            wantd = [[p for p in e if p < ks] or [e[0]] for e in erased]
            keep, rslots = rs.recover_batch_ragged(
                fragments, erased, want=wantd, part_blocks=src_nb,
                src_stride=src_stride, dst_stride=src_stride,
                out=torch.empty(
                    (S, max(len(w) for w in wantd),
                     (int(src_nb.max()) - 1) * src_stride + _BLOCK),
                    dtype=torch.uint8, device=dev))
            for s in range(S):
                for j, p in enumerate(rslots[s]):
                    if 0 <= p < ks and lost[s, p]:
                        view[s, p] = keep[s, j].data_ptr()
        view = np.where(used, view, np.uint64(0))
        lib, eng = L.lib(), L.engine(device)
        stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        u8p = ctypes.POINTER(ctypes.c_uint8)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        u64p = ctypes.POINTER(ctypes.c_uint64)

        def call(srcs, dests, tables, index, vw, n, col0, dp, dn):
            arrs = [np.ascontiguousarray(a, t) for a, t in
                    ((tables, np.uint8), (index, np.uint32), (vw, np.uint64),
                     (n, np.uint32), (col0, np.uint32), (dp, np.uint64),
                     (dn, np.uint32))]
            tb, ix, vw, n, col0, dp, dn = arrs
            L.check(lib.lizec_ec_encode_batch_view(
                eng, srcs, dests, tb.ctypes.data_as(u8p), tb.shape[0],
                ix.ctypes.data_as(u32p), vw.ctypes.data_as(u64p), ks,
                n.ctypes.data_as(u32p), kt, col0.ctypes.data_as(u32p),
                dp.ctypes.data_as(u64p), dn.ctypes.data_as(u32p), n.size,
                src_stride, dst_stride, stream),
                "lizec_ec_encode_batch_view")

        # data targets: one stripe per (chunk, wanted data part), one source
        # at the part's column, coefficient 1
        dsel = [(s, j) for s in range(S) for j in range(oc)
                if plan.slots[s, j] >= 0 and plan.dst_nb[s, j] and
                _data_index(target_slice, int(plan.slots[s, j])) is not None]
        if dsel:
            one = np.zeros((1, 32), np.uint8)
            lib.ec_init_tables(1, 1, np.ones(1, np.uint8).ctypes.data_as(u8p),
                               one.ctypes.data_as(u8p))
            ss = [s for s, _ in dsel]
            call(1, 1, one, np.zeros(len(dsel), np.uint32), view[ss], cb[ss],
                 [_data_index(target_slice, int(plan.slots[s, j]))
                  for s, j in dsel],
                 [dst[s, j] for s, j in dsel],
                 [plan.dst_nb[s, j] for s, j in dsel])
        # parity targets: one stripe per chunk, a table per distinct want set
        psets = [tuple(p for p in w
                       if _data_index(target_slice, p) is None) for w in wants]
        pc = max(len(p) for p in psets)
        if pc:
            distinct = sorted(set(psets))
            tables = np.zeros((len(distinct), 32 * kt * pc), np.uint8)
            for i, ps in enumerate(distinct):
                if not ps:
                    continue
                if st.is_xor(target_slice):
                    # all ones, as xor.py: parity = XOR of the data parts
                    tbl = np.zeros(32 * kt, np.uint8)
                    lib.ec_init_tables(
                        kt, 1, np.ones(kt, np.uint8).ctypes.data_as(u8p),
                        tbl.ctypes.data_as(u8p))
                else:
                    mt = st.parity_parts(target_slice)
                    tbl, parts = _pattern_table(
                        kt, mt, ((1 << mt) - 1) << kt,
                        sum(1 << p for p in ps))
                    assert tuple(parts) == ps
                tables[i, :tbl.size] = tbl
            index = [distinct.index(ps) for ps in psets]
            dp = np.zeros((S, pc), np.uint64)
            dn = np.zeros((S, pc), np.uint32)
            for s, ps in enumerate(psets):
                for l, p in enumerate(ps):
                    j = wants[s].index(p)
                    dp[s, l], dn[s, l] = dst[s, j], plan.dst_nb[s, j]
            if dn.any():
                call(kt, pc, tables, index, view, cb, np.zeros(S, np.uint32),
                     dp, dn)
        # `keep` may go now: the calls above are enqueued on the stream that
        # torch's allocator orders any reuse of that memory behind

    plan.run = run
    return plan


def _check_dst_stride(dst_stride):
    if dst_stride < _BLOCK or dst_stride % 4:
        raise ValueError(f"dst_stride={dst_stride} must be a multiple of 4 "
                         f"and at least {_BLOCK}")


def convert_parts(src_slice, fragments, chunk_blocks, target_slice, want,
                  out=None, src_erased=None, src_stride=_BLOCK,
                  dst_stride=_BLOCK, device=0):
    """Build the `want` parts of `target_slice` for a batch of chunks held
    as `src_slice`, in two lizec_ec_encode_batch_view calls (data parts,
    parity parts).

    fragments: one [S, Lmax] CUDA uint8 row view per part of the source
      slice (standard: 1; xorN: N+1, part 0 the parity; ec(k,m): k+m), blocks
      at src_stride, or None.  Only the data parts are read
      (view_columns), each as far as its chunk reaches.
    chunk_blocks: S block counts in 1..1024.
    want: a set of target parts, or one set per chunk.  A xorN target's
      part 0 is its parity.
    src_erased: ec source only — source parts that are missing (one set or
      one per chunk, at most m each).  Missing data parts are first rebuilt
      into scratch by ReedSolomon.recover_batch_ragged.
    out: optional [S, oc, span] CUDA uint8 tensor with contiguous rows,
      blocks at dst_stride; required unless dst_stride is 65536.
    Returns (out, slots [S, oc]): slots[s] lists chunk s's wanted parts in
    ascending order, -1 for an unused slot; of out[s, j] only the blocks the
    part has (slice_traits.number_of_blocks) are written.
    """
    _check_dst_stride(dst_stride)
    if out is None and dst_stride != _BLOCK:
        raise ValueError("out is required when dst_stride != 65536")
    plan = _prepare(src_slice, fragments, chunk_blocks, target_slice, want,
                    src_erased, src_stride, device)
    S, oc = plan.slots.shape
    top = int(plan.dst_nb.max())
    need = (top - 1) * dst_stride + _BLOCK if top else 0
    if out is None:
        out = torch.empty((S, oc, max(need, 1)), dtype=torch.uint8,
                          device=plan.dev)
    else:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or \
                not out.is_cuda or out.dim() != 3 or out.stride(2) != 1 or \
                tuple(out.shape[:2]) != (S, oc):
            raise ValueError(f"out must be a CUDA uint8 [S={S}, oc={oc}, "
                             f"span] tensor with contiguous rows")
        if out.shape[2] < need:
            raise ValueError(f"out: rows of {out.shape[2]} bytes cannot hold "
                             f"{top} blocks at stride {dst_stride} "
                             f"({need} bytes)")
        if out.data_ptr() % 4 or out.stride(0) % 4 or out.stride(1) % 4:
            raise ValueError("out: block data must be 4-byte aligned")
    dst = (np.uint64(out.data_ptr()) +
           np.arange(S, dtype=np.uint64)[:, None] * np.uint64(out.stride(0)) +
           np.arange(oc, dtype=np.uint64)[None, :] * np.uint64(out.stride(1)))
    if top:
        plan.run(dst, dst_stride)
    return out, plan.slots
