/* ec_kernel_view.h — sibling of ec_encode_ragged_kernel whose sources are a
 * CHUNK VIEW: the chunk's data held in another slice type, from which the
 * parts of the target slice are cut.
 *
 * This is what SliceRecoveryPlanner does when a part cannot be rebuilt from
 * its own slice (slice_recovery_planner.h:85-204): the chunk is read as
 * consecutive blocks from a standard copy, a xorN slice or an ec(k,m) of
 * another geometry (chunk_read_planner.h:36-58); a data part of the target is
 * every k-th of those blocks (kRecoverDataPart, :41-55) and a parity part is
 * computed over rows of k consecutive ones (kRecoverParityPart,
 * ec_read_plan.h:38-66, xor_read_plan.h:39).  It is the path every chunk
 * takes when a goal changes.
 *
 * A stripe's view is view_parts (= ks) addresses and one count n: chunk block
 * c < n is the 64 KiB at view[stripe][c % ks] + (c / ks) * src_stride, and
 * the blocks from n on are zeros.  In block row b the kernel's source j is
 * chunk block c0 + j with c0 = b * row_cols + col0[stripe]: row_cols is the
 * target's data-part count; a parity target has col0 = 0 and srcs = row_cols,
 * a data target has col0 = its index, srcs = 1 and a coefficient-1 table.
 *
 * Tile geometry, one tile per workgroup, block map, tbl_index, LDS table
 * staging, pipelined accumulation, SAL / DAL forms, dest_base passes and the
 * destination rule are those of ec_encode_ragged_kernel.  Only the source
 * side differs:
 *  - presence is monotone in j (source j is present iff c0 + j < n), so the
 *    source loop runs to min(srcs, n - c0) and tests no flag per source; a
 *    row that no source reaches is stored as zeros;
 *  - (part, block) of c0 come from one division per workgroup, on scalars;
 *    every further source advances them by increment-and-wrap, so there is no
 *    division per source and no per-lane address table.
 * Every condition compares scalars loaded at workgroup-uniform addresses, so
 * every branch is workgroup-uniform.
 */
#pragma once
#include "ec_kernel_ragged.h"

template <int D, int CH, bool SAL, bool DAL>
__global__ __launch_bounds__(kThreads) void ec_encode_view_kernel(
    int srcs, int dest_base,
    const uint8_t *__restrict__ tables_dev,    /* [ntables][dests_total][srcs][32] */
    const uint32_t *__restrict__ tbl_index,    /* [stripes] */
    const uint2 *__restrict__ block_map,       /* [gridDim.x / tiles per block] */
    const uint64_t *__restrict__ view_ptrs,    /* [stripes][view_parts] */
    uint32_t view_parts,
    const uint32_t *__restrict__ chunk_blocks, /* [stripes] */
    uint32_t row_cols,
    const uint32_t *__restrict__ col0,         /* [stripes] */
    const uint64_t *__restrict__ dst_ptrs,     /* [stripes][dests_total] */
    const uint32_t *__restrict__ dst_nblocks,  /* [stripes][dests_total] */
    int dests_total, uint32_t src_stride, uint32_t dst_stride) {
	constexpr uint32_t kTile = kChunkBytes * CH;
	static_assert(kECBlockBytes % kTile == 0, "a tile must not straddle");
	constexpr uint32_t kTilesPerBlock = kECBlockBytes / kTile;
	extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
	const uint32_t tid = threadIdx.x;

	/* tile -> (map entry, tile in block), as the ragged kernel */
	const uint32_t tile = xcd_remap(blockIdx.x, gridDim.x);
	const uint2 ent = block_map[tile / kTilesPerBlock];
	const uint32_t stripe = ent.x, blk = ent.y;
	const uint32_t in_blk = (tile % kTilesPerBlock) * kTile;
	const uint64_t *vp_tab = view_ptrs + (uint64_t)stripe * view_parts;
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

	/* the row's first chunk block, how many of its sources exist, and where
	 * the first one lives: the only division of the workgroup */
	const uint32_t n = chunk_blocks[stripe];
	const uint32_t c0 = blk * row_cols + col0[stripe];
	int cnt = 0;
	if (c0 < n) cnt = n - c0 < (uint32_t)srcs ? (int)(n - c0) : srcs;
	uint32_t vblk = c0 / view_parts;
	uint32_t vpart = c0 - vblk * view_parts;

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
	/* address of the next chunk block's tile, then one step round the view */
	auto next_src = [&]() {
		const uint8_t *sp = (const uint8_t *)vp_tab[vpart] +
		                    ((uint64_t)vblk * src_stride + in_blk);
		if (++vpart == view_parts) {
			vpart = 0;
			++vblk;
		}
		return sp;
	};
	if (cnt > 0) {
		const uint8_t *sp = next_src();
#pragma unroll
		for (int c = 0; c < CH; ++c)
			w[c] = ec_ld16<SAL>(sp + (lane_off + c * kChunkBytes));
	}
	/* stage this pass's rows of the stripe's table: [D][srcs][32] bytes,
	 * after the first source's loads are issued (ec_kernel_ragged.h) */
	{
		const uint8_t *src_tbl =
		    tables_dev +
		    ((size_t)tbl_index[stripe] * dests_total + dest_base) * srcs * 32;
		int nbytes = D * srcs * 32;
		for (int i = tid * 16; i < nbytes; i += kThreads * 16)
			*(uint4 *)(smem + i) = *(const uint4 *)(src_tbl + i);
	}
	__syncthreads();
	/* one source step, j < cnt: accumulate source j while source j+1's
	 * strips (more: it exists) are in flight */
	auto step = [&](int j, bool more) {
		if (more) {
			const uint8_t *spn = next_src();
#pragma unroll
			for (int c = 0; c < CH; ++c)
				wn[c] = ec_ld16<SAL>(spn + (lane_off + c * kChunkBytes));
		}
#pragma unroll
		for (int d = 0; d < D; ++d) {
			const uint8_t *tb = smem + ((size_t)d * srcs + j) * 32;
			T[d] = *(const uint4 *)tb;
			T6[d].x = *(const uint32_t *)(tb + 16);
		}
#pragma unroll
		for (int c = 0; c < CH; ++c)
			gf_macc_all_mr<D, CH>(acc, c, w[c], T, T6);
#pragma unroll
		for (int c = 0; c < CH; ++c) w[c] = wn[c];
	};
	/* presence being monotone, the loop bound is the only test: every source
	 * but the last has a successor to prefetch.  Not unrolled by hand: the
	 * ragged kernel's pair of steps, without that kernel's per-source
	 * branches between them, lets the scheduler keep a further set of
	 * strips in flight, which costs D = 1, 2 and 7 a wave per SIMD. */
	for (int j = 0; j < cnt; ++j) step(j, j + 1 < cnt);
#pragma unroll
	for (int d = 0; d < D; ++d) {
		if (!store[d]) continue;   /* workgroup-uniform */
		uint8_t *dp = (uint8_t *)dp_tab[d] + doff;
#pragma unroll
		for (int c = 0; c < CH; ++c)
			ec_st16<DAL>(dp + (lane_off + c * kChunkBytes), acc[d][c]);
	}
}
