"""The batched write gate — what hdd_write (hddspacemgr.cc:1899-2009) checks
and computes before it touches the disk, for many client writes at once.

One op is one packet: `size` bytes for [offset, offset + size) of one 64 KiB
block.  The gate verifies the CRC the client claims for the data, verifies a
partially overwritten block against its stored CRC, and returns the block's
new CRC; it writes nothing else.  Copying the data in and storing the CRC
stay with the caller.  include/lizec.h (lizec_write_gate_batch) has the
contract; gate_host is the same over host memory and needs no GPU."""
import ctypes

import numpy as np

from . import lib as L
from . import scrub

OK, BAD_DATA, BAD_BLOCK = 0, 1, 2     # LIZEC_GATE_*
SPARSE = 1                            # LIZEC_GATE_SPARSE

# lizec_write_op: 40 bytes, no padding
OP_DTYPE = np.dtype([("data", "<u8"), ("block", "<u8"), ("stored", "<u8"),
                     ("offset", "<u4"), ("size", "<u4"), ("crc", "<u4"),
                     ("reserved", "<u4")])
assert OP_DTYPE.itemsize == 40


def _address(buf):
    """Address of a torch tensor's or a numpy array's first byte."""
    return buf.data_ptr() if hasattr(buf, "data_ptr") else buf.ctypes.data


def _numel(buf):
    return buf.numel() if hasattr(buf, "numel") else buf.size


def image_blocks(image, fmt, slice_type):
    """64 KiB blocks a part-file image of this size holds."""
    data_off, _, bstride, _ = scrub.image_layout(fmt, slice_type)
    if fmt == "interleaved":
        return _numel(image) // bstride
    return max(0, _numel(image) - data_off) // bstride


def make_op(image, fmt, slice_type, block, offset, data, data_offset, size,
            crc):
    """One op: write data[data_offset : data_offset + size], for which the
    client claims `crc`, to [offset, offset + size) of block `block` of a
    part-file image in either on-disk format (scrub.image_layout).  image
    and data are flat uint8 buffers, CUDA tensors for gate_batch or numpy
    arrays for gate_host.  A block index at or past the image's last block
    gives block address 0: the block counts as zeros.  Returns a record of
    OP_DTYPE; ops_array() packs a list of them."""
    data_off, crc_off, bstride, cstride = scrub.image_layout(fmt, slice_type)
    if size and not 0 <= data_offset <= _numel(data) - size:
        raise ValueError("the op's data lies outside the data buffer")
    op = np.zeros((), OP_DTYPE)
    op["data"] = _address(data) + data_offset if size else 0
    if 0 <= block < image_blocks(image, fmt, slice_type):
        op["block"] = _address(image) + data_off + block * bstride
        op["stored"] = _address(image) + crc_off + block * cstride
    op["offset"] = offset
    op["size"] = size
    op["crc"] = crc
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
    """lizec_write_gate_host: the addresses in ops are host addresses.
    Returns (status int32[n], newcrc uint32[n]) as numpy arrays."""
    ops = ops_array(ops)
    n = ops.size
    status = np.empty(n, np.int32)
    newcrc = np.empty(n, np.uint32)
    L.check(L.lib().lizec_write_gate_host(
        ctypes.c_void_p(ops.ctypes.data), n, SPARSE if sparse else 0,
        ctypes.c_void_p(status.ctypes.data),
        ctypes.c_void_p(newcrc.ctypes.data)), "lizec_write_gate_host")
    return status, newcrc


def gate_batch(ops, sparse=False, device=0):
    """lizec_write_gate_batch on the current stream of `device`: the
    addresses in ops are device addresses.  Returns (status, newcrc), int32
    CUDA tensors [n]; newcrc holds the CRCs' bit patterns (view as uint32),
    as crc.crc32_blocks does.  Asynchronous, like the other batch calls."""
    import torch
    ops = ops_array(ops)
    n = ops.size
    status = torch.empty(n, dtype=torch.int32, device=f"cuda:{device}")
    newcrc = torch.empty(n, dtype=torch.int32, device=f"cuda:{device}")
    stream = torch.cuda.current_stream(device).cuda_stream
    L.check(L.lib().lizec_write_gate_batch(
        L.engine(device), ctypes.c_void_p(ops.ctypes.data), n,
        SPARSE if sparse else 0, ctypes.c_void_p(status.data_ptr()),
        ctypes.c_void_p(newcrc.data_ptr()), ctypes.c_void_p(stream)),
        "lizec_write_gate_batch")
    return status, newcrc

