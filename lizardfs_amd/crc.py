"""Per-block CRC32 — the chunkserver's read/write/scrub gate
(hddspacemgr.cc:1918-1920, :1525-1594, :2148-2212), batched on GPU.

Host-side scalar crc32/crc32_combine mirror common/crc.h:25-31 for the
protocol edges (packet CRCs, partial-block combines)."""
import ctypes

import numpy as np
import torch

from . import lib as L
from . import slice_traits


def crc32(data, seed=0):
    """Host scalar CRC-32 (zlib-compatible; crc.cc:113-151 semantics)."""
    b = bytes(data)
    return L.lib().lizec_crc32(seed, b, len(b))


def crc32_combine(crc1, crc2, len2):
    """crc.cc:207-224 semantics (crc of concatenation)."""
    return L.lib().lizec_crc32_combine(crc1, crc2, len2)


# lizec_crc32_batch's bound: its combine matrices cover zero runs of up to
# block_len / 2 < 2^26 bytes
MAX_BLOCK_LEN = 1 << 27


def crc32_blocks(buf, block_len=slice_traits.BLOCK_SIZE, seed=0, out=None,
                 device=None):
    """CRC32 of consecutive fixed-size blocks of a device buffer.

    buf: uint8 CUDA tensor, flat or any shape with numel % block_len == 0.
    Returns int32 CUDA tensor [nblocks] holding the CRCs (bit pattern; view
    as uint32).  block_len must be a multiple of 1024 below 2^27, and buf
    at least 4-byte aligned (lizec.h, lizec_crc32_batch).
    """
    if buf.dtype != torch.uint8 or not buf.is_cuda or not buf.is_contiguous():
        raise ValueError("buf must be a contiguous CUDA uint8 tensor")
    if block_len <= 0 or block_len % 1024 or block_len >= MAX_BLOCK_LEN:
        raise ValueError(f"block_len must be a multiple of 1024 below "
                         f"{MAX_BLOCK_LEN} (got {block_len})")
    if buf.data_ptr() % 4:
        raise ValueError(f"buf must be 4-byte aligned "
                         f"(address {buf.data_ptr():#x})")
    n = buf.numel()
    if n % block_len:
        raise ValueError("buffer size must be a multiple of block_len")
    nblocks = n // block_len
    dev = buf.device.index or 0
    if out is None:
        out = torch.empty(nblocks, dtype=torch.int32, device=buf.device)
    stream = torch.cuda.current_stream(dev).cuda_stream
    L.check(L.lib().lizec_crc32_batch(
        L.engine(dev), ctypes.c_void_p(buf.data_ptr()), block_len, nblocks,
        ctypes.c_uint32(seed), ctypes.c_void_p(out.data_ptr()),
        ctypes.c_void_p(stream)), "lizec_crc32_batch")
    return out


# lizec_crc32_ranges: a range is at most a block, a call at most 2^24
# ranges; its launch has at most 16384 workgroups of 4 waves, one range per
# wave at a time (lizec.h)
MAX_RANGE_LEN = slice_traits.BLOCK_SIZE
MAX_RANGES = 1 << 24
RANGES_GRID_WAVES = 16384 * 4


def crc32_ranges(buf, offsets, lengths, seed=0, out=None):
    """CRC32 of independent byte ranges of a device buffer:
    out[i] = crc32(seed, buf[offsets[i] : offsets[i] + lengths[i]]).

    buf: contiguous uint8 CUDA tensor, of any alignment.  offsets, lengths:
    integer arrays of equal size; a length is 0..65536 and a range of any
    byte alignment, but inside buf (checked here, on the host).  Ranges may
    overlap or repeat.  Returns an int32 CUDA tensor [n] holding the CRCs
    (bit pattern; view as uint32), as crc32_blocks does.  No ranges at all
    (n = 0) give an empty tensor without a call into the library.
    """
    if buf.dtype != torch.uint8 or not buf.is_cuda or not buf.is_contiguous():
        raise ValueError("buf must be a contiguous CUDA uint8 tensor")
    offs = np.asarray(offsets)
    lens = np.asarray(lengths)
    if offs.ndim != 1 or offs.shape != lens.shape or \
            offs.dtype.kind not in "iu" or lens.dtype.kind not in "iu":
        raise ValueError("offsets and lengths must be integer arrays of one "
                         "size")
    offs = offs.astype(np.int64)
    lens = lens.astype(np.int64)
    if (offs < 0).any() or (lens < 0).any() or \
            (offs + lens > buf.numel()).any():
        raise ValueError("a range lies outside buf")
    if (lens > MAX_RANGE_LEN).any():
        raise ValueError(f"a range is longer than {MAX_RANGE_LEN} bytes")
    n = int(offs.size)
    dev = buf.device.index or 0
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=buf.device)
    elif out.dtype != torch.int32 or not out.is_cuda or \
            not out.is_contiguous() or out.numel() != n:
        raise ValueError("out must be a contiguous CUDA int32 tensor [n]")
    if n == 0:
        return out            # the library refuses an empty call
    dptrs = (offs + buf.data_ptr()).astype(np.uint64)
    lens32 = lens.astype(np.uint32)
    stream = torch.cuda.current_stream(dev).cuda_stream
    L.check(L.lib().lizec_crc32_ranges(
        L.engine(dev), dptrs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
        lens32.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), n,
        ctypes.c_uint32(seed), ctypes.c_void_p(out.data_ptr()),
        ctypes.c_void_p(stream)), "lizec_crc32_ranges")
    return out
