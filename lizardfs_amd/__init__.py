"""lizardfs_amd — MI355X-native erasure-coding engine for the LizardFS
chunkserver EC hot path.

The compute path is liblizec.so (HIP/CDNA4 kernels behind the C ABI declared
in include/lizec.h, the reference's own ISA-L-shaped plugin seam).  This
package is the host-side mirror of the reference's EC surfaces:

  lizardfs_amd.slice_traits — Goal::Slice::Type / ChunkPartType algebra
  lizardfs_amd.ec           — batched ReedSolomon encode/decode on GPU
  lizardfs_amd.crc          — per-block CRC32 (GPU batch + host scalar)
  lizardfs_amd.convert      — parts of one slice type from a chunk held in
                              another (goal change)
  lizardfs_amd.chunkread    — the client read: block ranges of chunks
                              gathered from a slice's parts, lost parts
                              rebuilt on the way
  lizardfs_amd.chunkwrite   — the client write: parity and packet CRCs of
                              byte ranges written into a slice's blocks
  lizardfs_amd.writegate    — the batched hdd_write gate: byte-range data
                              and block CRC checks, new block CRCs
  lizardfs_amd.readgate     — the batched hdd_read gate: block CRC check and
                              READ_DATA payloads (CRC + bytes) of byte ranges

PyTorch supplies device memory and streams only; all byte-level compute is
the HIP library.  There is NO CPU fallback on the product path: using the
GPU APIs without liblizec.so or without an MI355X raises immediately.
"""
from . import slice_traits  # noqa: F401
from .lib import LizecError, gpu_count  # noqa: F401
from .lib import lib as load_lib  # noqa: F401
from . import ec  # noqa: F401
from . import crc  # noqa: F401
from . import writegate  # noqa: F401
from . import readgate  # noqa: F401
from . import chunkwrite  # noqa: F401

__all__ = ["slice_traits", "ec", "crc", "writegate", "readgate", "chunkwrite",
           "load_lib",
           "gpu_count", "LizecError"]
