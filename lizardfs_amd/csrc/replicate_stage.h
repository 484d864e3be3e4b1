/* replicate_stage.h — the two small kernels of the ragged streaming rebuild
 * (lizec_replicate_run_ragged): what a stage needs besides the ragged EC
 * kernel (ec_kernel_ragged.h) and the image CRC fill.
 *
 * Neither is on the critical path: the pipeline is bound by the PCIe copies
 * on both sides of them.  They exist to take API calls and a host pass out
 * of a stage — a memset and a copy per image header, a CRC pass over the
 * sources on the CPU — and are not tuned beyond the shapes below.
 *
 * replicate_header_kernel.  One workgroup per image slot of the stage.  A
 * wanted MooseFS image (address != 0) gets its header: header_size bytes of
 * zeros with the slot's signature (sig_len bytes, from the table uploaded
 * with the stage's metadata) at offset 0.  The CRC array inside the header
 * is filled afterwards by the CRC fill.  Thread t composes the 16-byte units
 * t, t + 256, ... and stores each with one plain 16-byte vector store: the
 * images are staged at 16-byte aligned addresses and header_size is a
 * multiple of 16, so no unit is shared with a neighbouring image.
 *
 * replicate_verify_kernel.  The source check of the rebuild: every block
 * that arrived is hashed and compared with the CRC that came with it, as
 * ReadOperationExecutor does (read_operation_executor.cc:261-263), modelled
 * on chunk_read_verify_kernel (read_verify.h).  One wave owns one (entry of
 * the source row map, source slot): block b of slot j of a chunk of the
 * stage; the map has one (chunk, block) entry per block row of the longest
 * source of every chunk (lizec_ragged_block_map over the source counts).
 * The wave's index is made uniform with readfirstlane, so everything it
 * looks up is a scalar load.  The block is checked iff the slot has a CRC
 * address (0 = not verified) and b < src_nblocks[chunk][j]; of any other
 * block neither a data byte nor a CRC byte is read.  The staged block is
 * 16-byte aligned and goes through crc_range_wave<false, false>
 * (crc_ranges.h); the expected value is read bytewise, big-endian, from the
 * staged CRC bytes at crc + 4 * b, at any alignment.  On a mismatch lane 0
 * ORs bit j into bad[chunk] with an ordinary atomic.
 *
 * Four waves per workgroup, one work item per wave, no stride loop; the only
 * barrier is the one behind the LDS table load, ahead of every return.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "crc_ranges.h"

constexpr int kReplHeaderThreads = 256;

__global__ __launch_bounds__(kReplHeaderThreads) void replicate_header_kernel(
    const uint64_t *__restrict__ images, /* [slots], 0 = not wanted */
    const uint8_t *__restrict__ sigs,    /* [slots][sig_len] */
    uint32_t sig_len, uint32_t header_size) {
	const uint64_t img = images[blockIdx.x];
	if (img == 0) return;
	const uint8_t *sig = sigs + (uint64_t)blockIdx.x * sig_len;
	for (uint32_t u = threadIdx.x * 16u; u < header_size;
	     u += kReplHeaderThreads * 16u) {
		uint4 w = make_uint4(0, 0, 0, 0);
		if (u < sig_len) {
			uint32_t v[4] = {0, 0, 0, 0};
			for (uint32_t k = 0; k < 16 && u + k < sig_len; ++k)
				v[k >> 2] |= (uint32_t)sig[u + k] << (8 * (k & 3));
			w = make_uint4(v[0], v[1], v[2], v[3]);
		}
		*(uint4 *)(img + u) = w;
	}
}

__global__ __launch_bounds__(kCrcRangesThreads) void replicate_verify_kernel(
    int srcs, uint64_t items,                 /* entries * srcs */
    const uint2 *__restrict__ src_map,        /* [entries]: chunk, block */
    const uint64_t *__restrict__ src_ptrs,    /* [chunks][srcs] */
    const uint64_t *__restrict__ crc_ptrs,    /* [chunks][srcs], 0 = unverified */
    const uint32_t *__restrict__ src_nblocks, /* [chunks][srcs] */
    const uint32_t *__restrict__ tab0, const uint32_t *__restrict__ mats_g,
    uint32_t *__restrict__ bad) {             /* [chunks], zeroed by the host */
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
	const uint2 ent = src_map[entry];
	const uint32_t chunk = ent.x, blk = ent.y;
	const uint64_t slot = (uint64_t)chunk * srcs + j;
	const uint64_t crc_addr = crc_ptrs[slot];
	if (crc_addr == 0 || blk >= src_nblocks[slot]) return;

	const uint64_t block = src_ptrs[slot] + (uint64_t)blk * 65536u;
	bool unused = false;
	const uint32_t have = crc_range_wave<false, false>(
	    block, 65536u, 0u, stabs, stabs + 256, lane, &unused);
	const crc_gbytes p = (crc_gbytes)(crc_addr + (uint64_t)blk * 4u);
	const uint32_t want = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) |
	                      ((uint32_t)p[2] << 8) | p[3];
	if (have != want && lane == 0) atomicOr(&bad[chunk], 1u << j);
}
