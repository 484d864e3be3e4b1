/* ec_kernel_write_degraded.h — ec_chunk_write_kernel (ec_kernel_write.h) for a
 * slice with lost parts: the parity of byte ranges written into the chunk
 * blocks of a slice whose fill columns may have to be rebuilt, in the parity
 * pass itself.
 *
 * ChunkWriter::fillStripe (mount/chunk_writer.cc:440-466) fills a partly
 * written row through readBlocks (:557-615), a planned read over whichever
 * parts have a location: a lost data part is rebuilt from the survivors
 * before computeParityBlock (:365-402) runs.  Everything involved is linear
 * over GF(2^8), so rebuild and encode fold into one coefficient table over
 * "new columns + old sources" (lizec_degraded_write_table), and one pass
 * reads every needed byte range once:
 *
 *   parity r of row b = XOR over the columns c NEW in the row of
 *                           tbl[r][c] * new_c
 *                     ^ XOR over the old slots j in the table's use mask
 *                           with b < old_nblocks[write][j] of
 *                           tbl[r][ks + j] * old_j
 *
 * where old_j is bytes [from, to) of block b of the part (data or parity)
 * behind slot j, at old[j] + b * old_stride + from.  A slot outside the mask
 * or at or past its count is neither loaded nor addressed.  tbl is the table
 * that tbl_index[write] names for the row: [0] for the write's first touched
 * row, [2] for its last where that is not the first, [1] for the rows
 * between; a scalar decision per workgroup.
 *
 * Tile map, xcd_remap, LDS table staging after the first loads are issued,
 * gf_macc_all_mr with the next source's loads in flight, dest_base passes,
 * tile sizes, the FAST and general forms and their load and store forms are
 * those of ec_chunk_write_kernel; ecw_issue, ecw_fix and ecw_store are used
 * as they are.  What differs is the source walk.  The up to ks + srcs
 * candidates of the row are gathered into one 64-bit presence mask with
 * scalar compares (the NEW columns of a row are one run of bits; an old slot
 * costs one count compare, and only if its mask bit is set), and the walk
 * takes the mask's set bits in ascending order: an absent candidate costs no
 * load, no address and no pipeline step, and the loads of the next PRESENT
 * candidate are in flight while the current one is accumulated.  The table
 * column of a source is its candidate number, not its position in the walk.
 * The loaded units move from the "next" registers to the "current" ones at
 * the end of a step, as in ec_chunk_write_kernel: a step whose two register
 * sets swap roles instead costs 30 to 110 VGPRs and a wave per SIMD.
 */
#pragma once
#include "ec_kernel_write.h"

template <int D, int CH, bool FAST>
__global__ __launch_bounds__(kThreads) void ec_chunk_write_degraded_kernel(
    int ks, int srcs, int dest_base, int rows_total,
    const uint8_t *__restrict__ tables_dev,   /* [ntables][rows_total]
                                                 [ks + srcs][32] */
    const uint32_t *__restrict__ use_masks,   /* [ntables] */
    const uint32_t *__restrict__ tbl_index,   /* [writes][3] */
    const uint4 *__restrict__ tile_map,       /* [gridDim.x]: write, row,
                                                 tile, row - first row */
    const lizec_chunk_write *__restrict__ writes,
    const uint64_t *__restrict__ old_ptrs,    /* [writes][srcs] */
    const uint32_t *__restrict__ old_nblocks, /* [writes][srcs] */
    const uint64_t *__restrict__ par_ptrs,    /* [writes][rows_total] */
    uint32_t old_stride) {
	constexpr uint32_t kTile = kChunkBytes * CH;
	extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
	const uint32_t tid = threadIdx.x;

	const uint4 ent = tile_map[xcd_remap(blockIdx.x, gridDim.x)];
	const uint32_t wi = ent.x, blk = ent.y;
	const lizec_chunk_write wr = writes[wi];
	const uint32_t off0 = ent.z * kTile;
	const uint32_t left = wr.to - wr.from - off0;   /* the map: off0 < size */
	const uint32_t n = left < kTile ? left : kTile;
	const uint32_t n16 = n & ~15u;
	const uint32_t tail = FAST ? 0u : n & 15u;

	/* this pass's parities: the tile's first byte, or 0 = not wanted */
	uint64_t dst[D];
	bool any = false;
	{
		const uint64_t *pp =
		    par_ptrs + (uint64_t)wi * rows_total + dest_base;
		/* par_stride is unused (and unchecked) if one row is touched */
		const uint64_t poff =
		    (ent.w ? (uint64_t)ent.w * wr.par_stride : 0) + off0;
#pragma unroll
		for (int d = 0; d < D; ++d) {
			const uint64_t p = pp[d];
			dst[d] = p ? p + poff : 0;
			any |= p != 0;
		}
	}
	if (!any) return;   /* whole workgroup, before the barrier */

	/* the row's table: first, middle or last touched row of the write */
	const uint32_t nc = (uint32_t)(ks + srcs);
	const uint32_t end = wr.first_block + wr.block_count;
	const uint32_t which =
	    ent.w == 0 ? 0u : (blk == (end - 1) / (uint32_t)ks ? 2u : 1u);
	const uint32_t ti = tbl_index[(uint64_t)wi * 3 + which];

	/* the candidates that are there: bit c < ks for a NEW column, bit
	 * ks + j for an old slot in the mask that has block blk */
	const uint64_t *op_tab = old_ptrs + (uint64_t)wi * srcs;
	const uint32_t c0 = blk * (uint32_t)ks;
	uint64_t pres;
	{
		const uint32_t lo = wr.first_block > c0 ? wr.first_block - c0 : 0u;
		const uint32_t hi = end - c0 < (uint32_t)ks ? end - c0 : (uint32_t)ks;
		pres = (((uint64_t)1 << hi) - 1) & ~(((uint64_t)1 << lo) - 1);
		const uint32_t *on_tab = old_nblocks + (uint64_t)wi * srcs;
		uint32_t m = use_masks[ti];
		if (srcs < 32) m &= (1u << srcs) - 1u;
		while (m) {
			const uint32_t j = (uint32_t)__builtin_ctz(m);
			m &= m - 1;
			if (blk < on_tab[j]) pres |= (uint64_t)1 << (ks + j);
		}
	}
	const uint64_t pres_all = pres;
	/* the tile's first byte of candidate i, which is there */
	auto source = [&](uint32_t i) -> uint64_t {
		if (i < (uint32_t)ks) {
			const uint32_t b = c0 + i - wr.first_block;
			return wr.data + (b ? (uint64_t)b * wr.data_stride : 0) + off0;
		}
		return op_tab[i - ks] + (uint64_t)blk * old_stride + wr.from + off0;
	};
	const uint32_t lane_off = tid * 16u;

	uint4 acc[D][CH];
#pragma unroll
	for (int d = 0; d < D; ++d)
#pragma unroll
		for (int c = 0; c < CH; ++c)
			acc[d][c] = make_uint4(0, 0, 0, 0);

	uint4 wa[CH], wb[CH];
	uint32_t ea[CH], eb[CH];
	uint4 T[D], T6[D];
#pragma unroll
	for (int c = 0; c < CH; ++c) {
		wa[c] = wb[c] = make_uint4(0, 0, 0, 0);
		ea[c] = eb[c] = 0;
	}
	/* cur: the candidate whose units are in flight or loaded, at cur_at */
	bool have = pres != 0;
	uint32_t cur = 0;
	uint64_t cur_at = 0;
	if (have) {
		cur = (uint32_t)__builtin_ctzll(pres);
		pres &= pres - 1;
		cur_at = source(cur);
		ecw_issue<CH, FAST>(cur_at, lane_off, n16, wa, ea);
	}
	/* stage this pass's rows of the row's table: [D][nc][32] bytes, after
	 * the first loads are issued (ec_kernel_ragged.h) */
	{
		const uint8_t *src_tbl =
		    tables_dev + ((size_t)ti * rows_total + dest_base) * nc * 32;
		int nbytes = D * (int)nc * 32;
		for (int i = tid * 16; i < nbytes; i += kThreads * 16)
			*(uint4 *)(smem + i) = *(const uint4 *)(src_tbl + i);
		__syncthreads();
	}
	/* one step: accumulate candidate cur out of (wa, ea) while the units of
	 * the next candidate that is there go into (wb, eb) */
	auto step = [&]() {
		const bool more = pres != 0;
		uint32_t nxt = 0;
		uint64_t nxt_at = 0;
		if (more) {
			nxt = (uint32_t)__builtin_ctzll(pres);
			pres &= pres - 1;
			nxt_at = source(nxt);
			ecw_issue<CH, FAST>(nxt_at, lane_off, n16, wb, eb);
		}
		if (!FAST) ecw_fix<CH>((uint32_t)cur_at & 3u, wa, ea);
#pragma unroll
		for (int d = 0; d < D; ++d) {
			const uint8_t *tb = smem + ((size_t)d * nc + cur) * 32;
			T[d] = *(const uint4 *)tb;
			T6[d].x = *(const uint32_t *)(tb + 16);
		}
#pragma unroll
		for (int c = 0; c < CH; ++c)
			gf_macc_all_mr<D, CH>(acc, c, wa[c], T, T6);
#pragma unroll
		for (int c = 0; c < CH; ++c) {
			wa[c] = wb[c];
			ea[c] = eb[c];
		}
		have = more;
		cur = nxt;
		cur_at = nxt_at;
	};
	while (have) step();
#pragma unroll
	for (int d = 0; d < D; ++d) {
		if (!dst[d]) continue;   /* workgroup-uniform */
		ecw_store<CH, FAST>(dst[d], lane_off, n16, acc[d]);
	}
	if (!FAST) {
		/* the bytes behind the last whole unit: lane i takes byte n16 + i
		 * through every candidate that is there, one table product per
		 * parity */
		if (tail) {
			const bool mine = tid < tail;
			const uint32_t at = n16 + tid;
			uint32_t a1[D];
#pragma unroll
			for (int d = 0; d < D; ++d) a1[d] = 0;
			uint64_t p = pres_all;
			while (p) {
				const uint32_t c = (uint32_t)__builtin_ctzll(p);
				p &= p - 1;
				const uint64_t s = source(c);
				uint32_t b = 0;
				if (mine) b = *(crc_gbytes)(s + at);
				const uint32_t f0 = b & 7u, f1 = (b >> 3) & 7u, f2 = b >> 6;
#pragma unroll
				for (int d = 0; d < D; ++d) {
					const uint8_t *tb = smem + ((size_t)d * nc + c) * 32;
					const uint4 t = *(const uint4 *)tb;
					const uint32_t t6 = *(const uint32_t *)(tb + 16);
					a1[d] = gf_macc_mr(a1[d], t, t6, f0, f1, f2);
				}
			}
#pragma unroll
			for (int d = 0; d < D; ++d) {
				if (!dst[d]) continue;
				if (mine) crc_store_byte((crc_gbytes_w)(dst[d] + at), a1[d]);
			}
		}
	}
}
