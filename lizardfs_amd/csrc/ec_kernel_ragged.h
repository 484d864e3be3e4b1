/* ec_kernel_ragged.h — sibling of ec_encode_strided_kernel for batches whose
 * parts differ in length: every stripe carries a block count per source and
 * per destination, and its own coefficient table.
 *
 * A chunk is 1..1024 blocks of 64 KiB and only a full one gives its parts a
 * common length: data part p of a chunk of n blocks has (n + k - p - 1) / k
 * blocks (slice_traits.h:311-316), so the last stripe row of a short chunk
 * has fewer than k data blocks and the missing ones are the zeros past the
 * end of the chunk.  ChunkReplicator::replicate works with exactly that, a
 * block count per chunk (chunk_replicator.cc:142-145).
 *
 * Same block-strided 64 KiB geometry, 4-byte-aligned forms (SAL / DAL),
 * tile sizes, one tile per workgroup, LDS table staging and pipelined
 * branchless accumulation as ec_encode_strided_kernel.  What differs:
 *  - tile -> (entry of the block map, tile in block).  The block map has one
 *    (stripe, block) entry per 64 KiB block row of the batch, built on the
 *    host (lizec_ragged_block_map); its address derives from blockIdx alone,
 *    so the lookup is a scalar load like the pointer-table reads, and no
 *    lane or workgroup searches for its stripe;
 *  - source j takes part in block b iff b < src_nblocks[stripe][j].  An
 *    absent source is skipped: neither its first load nor the prefetch
 *    issued one step ahead is executed, and its address is not even formed
 *    (it may be 0).  Skipping a term equals multiplying zeros, so the result
 *    is that of zero-padded parts — the reference's NULL-part rule
 *    (reed_solomon.h:79), with the other coefficients unchanged;
 *  - destination l is stored for block b iff b < dst_nblocks[stripe][l]; a
 *    block that no source covers is stored as zeros;
 *  - tbl_index[stripe] picks one of the packed tables; the workgroup stages
 *    its rows once anyway, so a table per stripe costs nothing extra;
 *  - a workgroup none of whose D destinations reaches block b (possible in
 *    the later passes of dests > 8) returns before it stages anything.
 * Every condition above compares scalars loaded at workgroup-uniform
 * addresses, so every branch is workgroup-uniform.
 */
#pragma once
#include "ec_kernel_strided.h"

template <int D, int CH, bool SAL, bool DAL>
__global__ __launch_bounds__(kThreads) void ec_encode_ragged_kernel(
    int srcs, int dest_base,
    const uint8_t *__restrict__ tables_dev,   /* [ntables][dests_total][srcs][32] */
    const uint32_t *__restrict__ tbl_index,   /* [stripes] */
    const uint2 *__restrict__ block_map,      /* [gridDim.x / tiles per block] */
    const uint64_t *__restrict__ src_ptrs,    /* [stripes][srcs]  */
    const uint32_t *__restrict__ src_nblocks, /* [stripes][srcs]  */
    const uint64_t *__restrict__ dst_ptrs,    /* [stripes][dests_total] */
    const uint32_t *__restrict__ dst_nblocks, /* [stripes][dests_total] */
    int dests_total, uint32_t src_stride, uint32_t dst_stride) {
	constexpr uint32_t kTile = kChunkBytes * CH;
	static_assert(kECBlockBytes % kTile == 0, "a tile must not straddle");
	constexpr uint32_t kTilesPerBlock = kECBlockBytes / kTile;
	extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
	const uint32_t tid = threadIdx.x;

	/* tile -> (map entry, tile in block); gridDim.x == entries * tiles per
	 * block, so every entry read lies inside the map */
	const uint32_t tile = xcd_remap(blockIdx.x, gridDim.x);
	const uint2 ent = block_map[tile / kTilesPerBlock];
	const uint32_t stripe = ent.x, blk = ent.y;
	const uint32_t in_blk = (tile % kTilesPerBlock) * kTile;
	const uint64_t *sp_tab = src_ptrs + (uint64_t)stripe * srcs;
	const uint32_t *sn_tab = src_nblocks + (uint64_t)stripe * srcs;
	const uint64_t *dp_tab =
	    dst_ptrs + (uint64_t)stripe * dests_total + dest_base;
	const uint32_t *dn_tab =
	    dst_nblocks + (uint64_t)stripe * dests_total + dest_base;

	bool store[D], any = false;
#pragma unroll
	for (int d = 0; d < D; ++d) {
		store[d] = blk < dn_tab[d];
		any |= store[d];
	}
	if (!any) return;   /* whole workgroup, before the barrier */

	/* workgroup-uniform 64-bit block offsets, per-lane 32-bit remainder */
	const uint64_t soff = (uint64_t)blk * src_stride + in_blk;
	const uint64_t doff = (uint64_t)blk * dst_stride + in_blk;
	const uint32_t lane_off = tid * 16u;

	uint4 acc[D][CH];
#pragma unroll
	for (int d = 0; d < D; ++d)
#pragma unroll
		for (int c = 0; c < CH; ++c)
			acc[d][c] = make_uint4(0, 0, 0, 0);

	uint4 w[CH], wn[CH];
	uint4 T[D], T6[D];
#pragma unroll
	for (int c = 0; c < CH; ++c) w[c] = wn[c] = make_uint4(0, 0, 0, 0);
	/* cur: source j has block blk, and its strips are in w */
	bool cur = blk < sn_tab[0];
	if (cur) {
		const uint8_t *sp = (const uint8_t *)sp_tab[0] + soff;
#pragma unroll
		for (int c = 0; c < CH; ++c)
			w[c] = ec_ld16<SAL>(sp + (lane_off + c * kChunkBytes));
	}
	/* stage this pass's rows of the stripe's table: [D][srcs][32] bytes.
	 * After the first source's loads are issued: the map lookup puts one more
	 * dependent scalar load in front of them than the strided kernel has,
	 * and the staging hides it. */
	{
		const uint8_t *src_tbl =
		    tables_dev +
		    ((size_t)tbl_index[stripe] * dests_total + dest_base) * srcs * 32;
		int nbytes = D * srcs * 32;
		for (int i = tid * 16; i < nbytes; i += kThreads * 16)
			*(uint4 *)(smem + i) = *(const uint4 *)(src_tbl + i);
	}
	__syncthreads();
	/* one source step: accumulate source j (if present) while source j+1's
	 * strips (if present) are in flight */
	auto step = [&](int j) {
		bool nxt = false;
		if (j + 1 < srcs) {
			nxt = blk < sn_tab[j + 1];
			if (nxt) {
				const uint8_t *spn = (const uint8_t *)sp_tab[j + 1] + soff;
#pragma unroll
				for (int c = 0; c < CH; ++c)
					wn[c] = ec_ld16<SAL>(spn + (lane_off + c * kChunkBytes));
			}
		}
		if (cur) {
#pragma unroll
			for (int d = 0; d < D; ++d) {
				const uint8_t *tb = smem + ((size_t)d * srcs + j) * 32;
				T[d] = *(const uint4 *)tb;
				T6[d].x = *(const uint32_t *)(tb + 16);
			}
#pragma unroll
			for (int c = 0; c < CH; ++c)
				gf_macc_all_mr<D, CH>(acc, c, w[c], T, T6);
		}
#pragma unroll
		for (int c = 0; c < CH; ++c) w[c] = wn[c];
		cur = nxt;
	};
	int j = 0;
	for (; j + 1 < srcs; j += 2) {
		step(j);
		step(j + 1);
	}
	if (j < srcs) step(j);
#pragma unroll
	for (int d = 0; d < D; ++d) {
		if (!store[d]) continue;   /* workgroup-uniform */
		uint8_t *dp = (uint8_t *)dp_tab[d] + doff;
#pragma unroll
		for (int c = 0; c < CH; ++c)
			ec_st16<DAL>(dp + (lane_off + c * kChunkBytes), acc[d][c]);
	}
}
