"""The batched read gate — what hdd_read (hddspacemgr.cc:1662-1727) does with
a block through hdd_read_crc_and_block (:1525-1608), for many client reads at
once.

One op is one READ: `size` bytes at `offset` of one 64 KiB block.  The gate
verifies the whole block against its stored CRC and writes the payload of
cstocl READ_DATA, [4-byte big-endian CRC][the bytes], in one pass over the
block.  include/lizec.h (lizec_read_gate_batch) has the contract; gate_host
is the same over host memory and needs no GPU."""
import ctypes

import numpy as np

from . import lib as L
from . import scrub
from .writegate import _address, _numel, image_blocks

OK, BAD_BLOCK = 0, 2                  # LIZEC_GATE_*
SPARSE = 1                            # LIZEC_GATE_SPARSE
BLOCK = 65536

# lizec_read_op: 32 bytes, no padding
OP_DTYPE = np.dtype([("block", "<u8"), ("stored", "<u8"), ("out", "<u8"),
                     ("offset", "<u4"), ("size", "<u4")])
assert OP_DTYPE.itemsize == 32


def make_op(image, fmt, slice_type, block, offset, size, out, out_offset):
    """One op: read [offset, offset + size) of block `block` of a part-file
    image in either on-disk format (scrub.image_layout) into the packet at
    out[out_offset : out_offset + 4 + size].  image and out are flat uint8
    buffers, CUDA tensors for gate_batch or numpy arrays for gate_host.  A
    block index at or past the image's last block gives block address 0:
    the block reads as zeros.  Returns a record of OP_DTYPE; ops_array()
    packs a list of them."""
    data_off, crc_off, bstride, cstride = scrub.image_layout(fmt, slice_type)
    if not 0 <= out_offset <= _numel(out) - 4 - size:
        raise ValueError("the op's packet lies outside the output buffer")
    op = np.zeros((), OP_DTYPE)
    if 0 <= block < image_blocks(image, fmt, slice_type):
        op["block"] = _address(image) + data_off + block * bstride
        op["stored"] = _address(image) + crc_off + block * cstride
    op["out"] = _address(out) + out_offset
    op["offset"] = offset
    op["size"] = size
    return op


def ops_array(ops):
    """Pack records (or an array) of OP_DTYPE into one contiguous array."""
    if isinstance(ops, np.ndarray) and ops.dtype == OP_DTYPE:
        return np.ascontiguousarray(ops.reshape(-1))
    out = np.zeros(len(ops), OP_DTYPE)
    for i, op in enumerate(ops):
        out[i] = op
    return out


def gate_host(ops, sparse=False):
    """lizec_read_gate_host: the addresses in ops are host addresses; the
    packets are written there.  Returns status, int32[n]."""
    ops = ops_array(ops)
    n = ops.size
    status = np.empty(n, np.int32)
    L.check(L.lib().lizec_read_gate_host(
        ctypes.c_void_p(ops.ctypes.data), n, SPARSE if sparse else 0,
        ctypes.c_void_p(status.ctypes.data)), "lizec_read_gate_host")
    return status


def gate_batch(ops, sparse=False, device=0):
    """lizec_read_gate_batch on the current stream of `device`: the addresses
    in ops are device addresses; the packets are written there.  Returns
    status, an int32 CUDA tensor [n].  Asynchronous, like the other batch
    calls: packets and status are ready when the stream gets there."""
    import torch
    ops = ops_array(ops)
    n = ops.size
    status = torch.empty(n, dtype=torch.int32, device=f"cuda:{device}")
    stream = torch.cuda.current_stream(device).cuda_stream
    L.check(L.lib().lizec_read_gate_batch(
        L.engine(device), ctypes.c_void_p(ops.ctypes.data), n,
        SPARSE if sparse else 0, ctypes.c_void_p(status.data_ptr()),
        ctypes.c_void_p(stream)), "lizec_read_gate_batch")
    return status


def read_packets(image, fmt, slice_type, requests, sparse=None):
    """The READ_DATA payloads of `requests`, (block, offset, size) each, over
    one part-file image, laid end to end in one uint8 buffer — what a
    chunkserver worker hands to its socket.  Returns (packets, starts,
    status): packet i is packets[starts[i] : starts[i] + 4 + size_i].  A
    CUDA image goes through gate_batch (packets and status are CUDA tensors,
    ready when the current stream gets there), a numpy image through
    gate_host.  sparse defaults to the format's own rule: INTERLEAVED has
    it, MooseFS does not.  A packet whose status is BAD_BLOCK must not be
    sent."""
    if sparse is None:
        sparse = fmt == "interleaved"
    sizes = np.array([r[2] for r in requests], np.int64)
    starts = np.zeros(len(requests), np.int64)
    np.cumsum(sizes[:-1] + 4, out=starts[1:])
    total = int(sizes.sum()) + 4 * len(requests)
    if hasattr(image, "data_ptr"):
        import torch
        packets = torch.empty(total, dtype=torch.uint8, device=image.device)
    else:
        packets = np.empty(total, np.uint8)
    ops = ops_array([make_op(image, fmt, slice_type, b, off, size, packets,
                             int(at))
                     for (b, off, size), at in zip(requests, starts)])
    if hasattr(image, "data_ptr"):
        status = gate_batch(ops, sparse=sparse, device=image.device.index or 0)
    else:
        status = gate_host(ops, sparse=sparse)
    return packets, starts, status
