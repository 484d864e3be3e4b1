/* read_verify.h — the CRC check of the CLIENT READ: every source block that
 * ec_chunk_read_kernel (ec_kernel_read.h) is about to load is hashed and
 * compared with the CRC that came with it, as ReadOperationExecutor does for
 * every block it receives (read_operation_executor.cc:261-263) before
 * ChunkReader decodes anything; a part with a bad block is reported, as
 * ChunkReader::readData records it in crcErrors_ (chunk_reader.cc:135-137).
 *
 * Hash only: the data movement stays in the read kernel, which runs behind
 * this one on the same stream and is not changed.  The wave-per-block walk
 * without a copy is the cheap half of the read gate (profiles/READ_GATE.md),
 * and the tile kernel's lane layout (16-byte units 4 KiB apart) would need a
 * 256-lane combine per tile and source to carry a CRC.
 *
 * One wave owns one (map entry, source slot): block row b of slot j of a
 * read.  It reads the row map and the slot_col / row_col / range /
 * src_nblocks arrays that the read call uploads anyway, all at wave-uniform
 * addresses (the wave's index is made uniform with readfirstlane, as in
 * read_gate.h), and checks the block iff
 *  - the slot has a CRC address (0 = not verified),
 *  - b < src_nblocks[read][j],
 *  - the read kernel loads it: the column the slot backs is requested in
 *    row b, or some lost column (any table row's) is requested in row b —
 *    the union over the passes of that kernel's `wanted`.
 * Such a block is checked exactly once; of any other block neither a data
 * byte nor a CRC byte is read.
 *
 * The block's 65536 bytes (4-byte aligned, as the read call requires) go
 * through crc_range_wave<false, false> (crc_ranges.h): up to 12 head bytes,
 * aligned 16-byte units, up to 12 tail bytes, nothing outside the block.
 * The expected value is four bytes, big-endian, read bytewise at
 * crc + b * crc_stride at any alignment.  On a mismatch lane 0 ORs bit j
 * into bad[read].  There is no sparse-block rule: that is the chunkserver's
 * (hddspacemgr.cc:1556-1596), the client compares unconditionally.
 *
 * Four waves per workgroup, exactly one work item per wave, no stride loop:
 * ceil(entries * srcs / 4) workgroups, at most entries * 8 <= 2^31 - 1 by
 * the read call's own bound.  The work item's index needs 64 bits.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "crc_ranges.h"

__global__ __launch_bounds__(kCrcRangesThreads) void chunk_read_verify_kernel(
    int srcs, int rows_total, uint64_t items, /* entries * srcs */
    const uint2 *__restrict__ block_map,      /* [entries]: read, block row */
    const uint64_t *__restrict__ src_ptrs,    /* [reads][srcs] */
    const uint64_t *__restrict__ crc_ptrs,    /* [reads][srcs], 0 = unverified */
    const uint32_t *__restrict__ src_nblocks, /* [reads][srcs] */
    const uint32_t *__restrict__ slot_col,    /* [reads][srcs] */
    const uint32_t *__restrict__ row_col,     /* [reads][rows_total] */
    uint32_t view_parts,
    const uint2 *__restrict__ range,          /* [reads]: first, count */
    uint32_t src_stride, uint32_t crc_stride,
    const uint32_t *__restrict__ tab0, const uint32_t *__restrict__ mats_g,
    uint32_t *__restrict__ bad) {             /* [reads], zeroed by the host */
	__shared__ __attribute__((aligned(16))) uint32_t stabs[kCrcRangesLdsWords];
	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const int lane = threadIdx.x & 63;
	for (int k = threadIdx.x; k < 256; k += kCrcRangesThreads)
		stabs[k] = tab0[k];
	for (int k = threadIdx.x; k < kCrcRangesMats * 32; k += kCrcRangesThreads)
		stabs[256 + k] = mats_g[k];
	__syncthreads();   /* the only barrier: every return is behind it */
	const uint64_t item = (uint64_t)blockIdx.x * 4 + wave;
	if (item >= items) return;
	const uint32_t entry = (uint32_t)(item / (uint32_t)srcs);
	const uint32_t j = (uint32_t)(item - (uint64_t)entry * (uint32_t)srcs);
	const uint2 ent = block_map[entry];
	const uint32_t read = ent.x, blk = ent.y;
	const uint64_t slot = (uint64_t)read * srcs + j;
	const uint64_t crc_addr = crc_ptrs[slot];
	if (crc_addr == 0 || blk >= src_nblocks[slot]) return;

	/* the requested columns of this row, as ec_chunk_read_kernel cuts them */
	const uint2 rg = range[read];
	const uint32_t first = rg.x, end = rg.x + rg.y;
	const uint32_t c0 = blk * view_parts;
	const uint32_t lo = first > c0 ? first - c0 : 0;
	const uint32_t hi = end - c0 < view_parts ? end - c0 : view_parts;
	const uint32_t width = hi - lo;
	/* kReadNoColumn (0xFFFFFFFF) - lo wraps far above any width */
	auto requested = [&](uint32_t col) { return col - lo < width; };
	bool loaded = requested(slot_col[slot]);
	const uint32_t *rc_tab = row_col + (uint64_t)read * rows_total;
	for (int r = 0; r < rows_total && !loaded; ++r) loaded = requested(rc_tab[r]);
	if (!loaded) return;

	const uint64_t block = src_ptrs[slot] + (uint64_t)blk * src_stride;
	bool unused = false;
	const uint32_t have = crc_range_wave<false, false>(
	    block, 65536u, 0u, stabs, stabs + 256, lane, &unused);
	const crc_gbytes p = (crc_gbytes)(crc_addr + (uint64_t)blk * crc_stride);
	const uint32_t want = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) |
	                      ((uint32_t)p[2] << 8) | p[3];
	if (have != want && lane == 0) atomicOr(&bad[read], 1u << j);
}
