/* ec_kernel_read.h — sibling of ec_encode_view_kernel for the CLIENT READ:
 * chunk blocks [first, first + count) gathered from the parts of one slice,
 * the blocks of lost parts rebuilt on the way.
 *
 * This is ChunkReader::readData (chunk_reader.cc:85-131) in one pass: the
 * slice's data parts interleave the chunk round-robin (chunk block c is row
 * c / ks, column c % ks; ChunkReadPlanner, chunk_read_planner.h:86-162), a
 * lost part is recomputed from the others (ECReadPlan::recoverParts,
 * ec_read_plan.h:113-146; XorReadPlan::postProcessRead,
 * xor_read_plan.h:77-126) and BlockConverter (chunk_read_planner.h:36-58)
 * copies part blocks back into chunk order.  Here a source tile is loaded
 * once and used twice: stored straight to the output block of the column it
 * backs, from the registers it was loaded into and with no GF multiply, and
 * accumulated into the rows of the lost columns.
 *
 * Tile geometry, one tile per workgroup, xcd_remap, the host-built map (one
 * entry per (read, block row) that the read's range touches), tbl_index, LDS
 * table staging after the first loads are issued, pipelined accumulation
 * through gf_macc_all_mr, SAL / DAL forms and dest_base passes are those of
 * ec_encode_ragged_kernel; so is the presence rule (source j has block b iff
 * b < src_nblocks[read][j]; an absent source is neither loaded nor
 * addressed).  What differs is the row-wise work.  In block row b the
 * requested columns are [lo, hi), clipped from the read's range.  Then
 *  - slot j COPIES iff this is pass 0 and the column it backs
 *    (slot_col[read][j], built on the host from col_map) lies in [lo, hi);
 *    an absent copying slot stores zeros — the padding of
 *    SliceReadPlan::postProcessRead (slice_read_plan.h:94-105);
 *  - accumulator d of the pass is STORED iff the column that table row
 *    dest_base + d stands for (row_col[read][dest_base + d]) lies in
 *    [lo, hi); the row ACCUMULATES iff any of the pass's D is stored;
 *  - slot j is LOADED iff it is present and copies or the row accumulates:
 *    a healthy row reads only the requested columns, and a row whose lost
 *    columns all lie outside the range reads no parity;
 *  - a pass other than 0 none of whose rows is stored returns at once;
 *  - D = 0 is the pure gather of a call without tables (rows == 0).
 * Columns outside [lo, hi) are never stored.  Every condition above compares
 * scalars loaded at workgroup-uniform addresses, so every branch is
 * workgroup-uniform, and nothing is searched: both inverse maps come from
 * the host.  Output block offsets are 64-bit.
 */
#pragma once
#include "ec_kernel_ragged.h"

constexpr uint32_t kReadNoColumn = 0xFFFFFFFFu;

template <int D, int CH, bool SAL, bool DAL>
__global__ __launch_bounds__(kThreads) void ec_chunk_read_kernel(
    int srcs, int dest_base, int rows_total,
    const uint8_t *__restrict__ tables_dev,   /* [ntables][rows_total][srcs][32] */
    const uint32_t *__restrict__ tbl_index,   /* [reads] */
    const uint2 *__restrict__ block_map,      /* [gridDim.x / tiles per block] */
    const uint64_t *__restrict__ src_ptrs,    /* [reads][srcs] */
    const uint32_t *__restrict__ src_nblocks, /* [reads][srcs] */
    const uint32_t *__restrict__ slot_col,    /* [reads][srcs] */
    const uint32_t *__restrict__ row_col,     /* [reads][rows_total] */
    uint32_t view_parts,
    const uint2 *__restrict__ range,          /* [reads]: first, count */
    const uint64_t *__restrict__ dst_ptrs,    /* [reads] */
    uint32_t src_stride, uint32_t dst_stride) {
	constexpr uint32_t kTile = kChunkBytes * CH;
	static_assert(kECBlockBytes % kTile == 0, "a tile must not straddle");
	constexpr uint32_t kTilesPerBlock = kECBlockBytes / kTile;
	constexpr int DA = D ? D : 1;   /* no zero-length arrays */
	extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
	const uint32_t tid = threadIdx.x;

	/* tile -> (map entry, tile in block), as the ragged kernel */
	const uint32_t tile = xcd_remap(blockIdx.x, gridDim.x);
	const uint2 ent = block_map[tile / kTilesPerBlock];
	const uint32_t read = ent.x, blk = ent.y;
	const uint32_t in_blk = (tile % kTilesPerBlock) * kTile;
	const uint64_t *sp_tab = src_ptrs + (uint64_t)read * srcs;
	const uint32_t *sn_tab = src_nblocks + (uint64_t)read * srcs;
	const uint32_t *sc_tab = slot_col + (uint64_t)read * srcs;

	/* the requested columns of this row: [lo, lo + width).  The map holds
	 * only rows that the range touches, so c0 < end and lo < view_parts. */
	const uint2 rg = range[read];
	const uint32_t first = rg.x, end = rg.x + rg.y;
	const uint32_t c0 = blk * view_parts;
	const uint32_t lo = first > c0 ? first - c0 : 0;
	const uint32_t hi = end - c0 < view_parts ? end - c0 : view_parts;
	const uint32_t width = hi - lo;
	/* kReadNoColumn - lo wraps far above any width */
	auto requested = [&](uint32_t col) { return col - lo < width; };

	uint32_t rcol[DA];
	bool store[DA], any = false;
	if constexpr (D > 0) {
		const uint32_t *rc_tab =
		    row_col + (uint64_t)read * rows_total + dest_base;
#pragma unroll
		for (int d = 0; d < D; ++d) {
			rcol[d] = rc_tab[d];
			store[d] = requested(rcol[d]);
			any |= store[d];
		}
	}
	const bool copies = dest_base == 0;
	if (!copies && !any) return;   /* whole workgroup, before the barrier */

	/* output block i = c0 + column - first lies at dst + i * dst_stride */
	uint8_t *const out = (uint8_t *)dst_ptrs[read] + in_blk;
	auto out_block = [&](uint32_t col) {
		return out + (uint64_t)(c0 + col - first) * dst_stride;
	};
	const uint64_t soff = (uint64_t)blk * src_stride + in_blk;
	const uint32_t lane_off = tid * 16u;

	uint4 acc[DA][CH];
#pragma unroll
	for (int d = 0; d < DA; ++d)
#pragma unroll
		for (int c = 0; c < CH; ++c)
			acc[d][c] = make_uint4(0, 0, 0, 0);

	uint4 w[CH], wn[CH];
	uint4 T[DA], T6[DA];
#pragma unroll
	for (int c = 0; c < CH; ++c) w[c] = wn[c] = make_uint4(0, 0, 0, 0);
	/* slot j's strips are wanted: it has block blk, and a use for it */
	auto wanted = [&](int j) {
		return blk < sn_tab[j] && (any || (copies && requested(sc_tab[j])));
	};
	/* cur: slot j's strips are in w */
	bool cur = wanted(0);
	if (cur) {
		const uint8_t *sp = (const uint8_t *)sp_tab[0] + soff;
#pragma unroll
		for (int c = 0; c < CH; ++c)
			w[c] = ec_ld16<SAL>(sp + (lane_off + c * kChunkBytes));
	}
	/* stage this pass's rows of the read's table: [D][srcs][32] bytes, after
	 * the first loads are issued (ec_kernel_ragged.h); a row that
	 * accumulates nothing stages nothing */
	if constexpr (D > 0) {
		if (any) {
			const uint8_t *src_tbl =
			    tables_dev +
			    ((size_t)tbl_index[read] * rows_total + dest_base) * srcs * 32;
			int nbytes = D * srcs * 32;
			for (int i = tid * 16; i < nbytes; i += kThreads * 16)
				*(uint4 *)(smem + i) = *(const uint4 *)(src_tbl + i);
			__syncthreads();   /* `any` is workgroup-uniform */
		}
	}
	/* one slot step: copy and accumulate slot j (as far as each applies)
	 * while slot j+1's strips (if wanted) are in flight */
	auto step = [&](int j) {
		bool nxt = false;
		if (j + 1 < srcs) {
			nxt = wanted(j + 1);
			if (nxt) {
				const uint8_t *spn = (const uint8_t *)sp_tab[j + 1] + soff;
#pragma unroll
				for (int c = 0; c < CH; ++c)
					wn[c] = ec_ld16<SAL>(spn + (lane_off + c * kChunkBytes));
			}
		}
		if (copies) {
			const uint32_t col = sc_tab[j];
			if (requested(col)) {
				/* wanted(j) holds iff the slot is present; w is stale
				 * otherwise, and the block is the zeros past its part */
				uint8_t *dp = out_block(col);
#pragma unroll
				for (int c = 0; c < CH; ++c)
					ec_st16<DAL>(dp + (lane_off + c * kChunkBytes),
					             cur ? w[c] : make_uint4(0, 0, 0, 0));
			}
		}
		if constexpr (D > 0) {
			if (any && cur) {
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
	if constexpr (D > 0) {
#pragma unroll
		for (int d = 0; d < D; ++d) {
			if (!store[d]) continue;   /* workgroup-uniform */
			uint8_t *dp = out_block(rcol[d]);
#pragma unroll
			for (int c = 0; c < CH; ++c)
				ec_st16<DAL>(dp + (lane_off + c * kChunkBytes), acc[d][c]);
		}
	}
}
