/* read_gate.h — the batched hdd_read gate: verify a 64 KiB block against its
 * stored CRC and emit [4-byte big-endian CRC][bytes] for any byte range of
 * it (hddspacemgr.cc:1662-1727 over :1525-1608), in ONE pass over the block.
 *
 * One wave owns one op and with it the three ranges of its block:
 *
 *   pre   block[0, offset)               hashed
 *   mid   block[offset, offset + size)   hashed and copied to out + 4
 *   post  block[offset + size, 65536)    hashed
 *
 * Each goes through crc_range_wave (crc_ranges.h): head bytes, aligned
 * 16-byte units folded, tail bytes — a range that is empty is skipped.  The
 * mid pass stores what it has loaded: the units from the registers the fold
 * reads them from, head and tail bytes as lane 0 walks them.  The source
 * units are 16-byte aligned, the packet's data starts at out + 4, so the
 * copies sit at (out + 4 - block - offset) mod 16 = d, the same for every
 * unit of the op: d = 0 stores 16 bytes, another multiple of 4 stores a
 * 16-byte vector that promises 4-byte alignment, anything else 16 single
 * bytes (crc_store_unit).  The form is wave-uniform, so the branch on it is
 * a scalar one.
 *
 * The same wave then splices the three CRCs into the block's (crc_splice64k),
 * reads the four stored bytes, applies the INTERLEAVED sparse rule where the
 * flag asks for it (the OR of the block's bytes comes out of the same pass),
 * and lane 0 writes the packet's CRC bytes and the status: one launch, no
 * finishing kernel, and nothing in scratch but the op table.
 *
 * One instance of the walk serves all three ranges (a loop, not three
 * inlined copies): `form` is kCrcCopyNone for pre and post.
 *
 * A past-end op (block == 0) hashes nothing: its packet is the CRC of `size`
 * zero bytes from the matrix bank and `size` zero bytes, stored in the same
 * three forms as if the block lay at address 0.
 *
 * The op table is read at wave-uniform addresses (the wave's index is made
 * uniform with readfirstlane), the next op's entry while this one runs.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/lizec.h"
#include "crc_ranges.h"

/* `len` zero bytes at dst, placed as the copy of a range at `vsrc` would be:
 * bytes up to the first 16-byte boundary of vsrc, units, bytes behind the
 * last unit.  form = crc_copy_form(dst, vsrc). */
__device__ __forceinline__ void read_gate_zero_fill(uint64_t dst, uint32_t vsrc,
                                                    uint32_t len, uint32_t form,
                                                    int lane) {
	const uint32_t to16 = (0u - vsrc) & 15u;
	const uint32_t head = to16 < len ? to16 : len;
	const uint32_t units = (len - head) >> 4;
	const uint32_t tail = (len - head) & 15u;
	const crc_gbytes_w b = (crc_gbytes_w)dst;
	const crc_u32x4 zero = {0u, 0u, 0u, 0u};
	if ((uint32_t)lane < head) b[lane] = 0;
	for (uint32_t u = (uint32_t)lane; u < units; u += 64)
		crc_store_unit(dst + head + ((uint64_t)u << 4), form, zero);
	if ((uint32_t)lane < tail) b[head + (units << 4) + lane] = 0;
}

__device__ __forceinline__ uint64_t read_gate_uniform(uint64_t v) {
	const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
	const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
	return ((uint64_t)hi << 32) | lo;
}

/* One wave per op, grid stride.  SPARSE: LIZEC_GATE_SPARSE is set (the pass
 * then carries the OR of the block's bytes).  Writes status[i] and the
 * 4 + size bytes of each packet, nothing else. */
template <bool SPARSE>
__global__ __launch_bounds__(kCrcRangesThreads) void read_gate_kernel(
    const lizec_read_op *__restrict__ ops, uint32_t n,
    const uint32_t *__restrict__ tab0, const uint32_t *__restrict__ mats_g,
    int32_t *__restrict__ status) {
	__shared__ __attribute__((aligned(16))) uint32_t stabs[kCrcRangesLdsWords];
	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const int lane = threadIdx.x & 63;
	const uint32_t stride = gridDim.x * 4;
	uint32_t i = blockIdx.x * 4 + wave;
	lizec_read_op op = {0, 0, 0, 0, 0};
	if (i < n) op = ops[i];
	for (int k = threadIdx.x; k < 256; k += kCrcRangesThreads)
		stabs[k] = tab0[k];
	for (int k = threadIdx.x; k < kCrcRangesMats * 32; k += kCrcRangesThreads)
		stabs[256 + k] = mats_g[k];
	__syncthreads();
	const uint32_t *T0 = stabs, *mats = stabs + 256;
	while (i < n) {
		/* n <= 2^24 and stride <= 2^16: no wrap */
		const uint32_t nx = i + stride;
		lizec_read_op nop = {0, 0, 0, 0, 0};
		if (nx < n) nop = ops[nx];
		const uint64_t block = read_gate_uniform(op.block);
		const uint64_t out = read_gate_uniform(op.out);
		const uint32_t offset = __builtin_amdgcn_readfirstlane(op.offset);
		const uint32_t size = __builtin_amdgcn_readfirstlane(op.size);
		const uint64_t data = out + 4;
		const uint32_t form = crc_copy_form(data, block + offset);
		int32_t st = LIZEC_GATE_OK;
		uint32_t crc;
		if (block == 0) {
			read_gate_zero_fill(data, offset, size, form, lane);
			crc = crc_zeroblock0(size, mats);
		} else {
			const uint32_t end = offset + size;
			uint32_t pre = 0, mid = 0, post = 0;
			bool nz = false;
#pragma unroll 1
			for (int r = 0; r < 3; ++r) {
				const uint32_t lo = r == 0 ? 0u : r == 1 ? offset : end;
				const uint32_t hi = r == 0 ? offset : r == 1 ? end : 65536u;
				if (lo == hi) continue;        /* crc32 of nothing is 0 */
				bool any = false;
				const uint32_t c = crc_range_wave<SPARSE, true>(
				    block + lo, hi - lo, 0u, T0, mats, lane, &any, data,
				    r == 1 ? form : (uint32_t)kCrcCopyNone);
				nz |= any;
				if (r == 0)
					pre = c;
				else if (r == 1)
					mid = c;
				else
					post = c;
			}
			const uint32_t have =
			    crc_splice64k(pre, offset, mid, size, post, mats);
			const crc_gbytes p = (crc_gbytes)read_gate_uniform(op.stored);
			uint32_t blk = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) |
			               ((uint32_t)p[2] << 8) | p[3];
			if (SPARSE && blk == 0) {
				/* :1571-1587: not checked; a zero block's CRC is recomputed */
				if (!nz) blk = crc_zeroblock0(65536u, mats);
			} else if (blk != have) {
				st = LIZEC_GATE_BAD_BLOCK;
			}
			/* :1711-1712 passes the block's CRC through, :1718 hashes */
			crc = (offset == 0 && size == 65536u) ? blk : mid;
			if (st != LIZEC_GATE_OK) crc = 0;
		}
		if (lane == 0) {
			const crc_gbytes_w o = (crc_gbytes_w)out;
			crc_store_byte(o, crc >> 24);     /* out has any alignment */
			crc_store_byte(o + 1, crc >> 16);
			crc_store_byte(o + 2, crc >> 8);
			crc_store_byte(o + 3, crc);
			status[i] = st;
		}
		i = nx;
		op = nop;
	}
}
