/* ec_kernel_multi.h — multi-table sibling of ec_encode_kernel (ec_kernel.h):
 * every stripe of the batch names its own coefficient table, so one launch
 * covers a batch of mixed erasure patterns (replicator rebuild after a disk
 * loss, chunk_replicator.cc:139-196; degraded reads, ec_read_plan.h:113-146
 * — each chunk / read operation carries its own pattern).
 *
 * Same tile geometry, XCD remap, non-temporal loads/stores, pipelined
 * branchless full-tile path and guarded ragged-tail path as the product
 * configuration of ec_encode_kernel (mixed-radix tables, gf_macc_all_mr).
 * What differs:
 *   - tables_dev holds `ntables` packed tables of dests_total*srcs*32 bytes
 *     each; tbl_index[stripe] picks one.  The block stages rows
 *     [dest_base, dest_base+D) of that table into LDS, and restages inside
 *     the grid-stride loop only when the next tile's index differs from the
 *     staged one (block-uniform: the condition depends on the tile alone).
 *   - a destination whose device address is 0 is not stored (wave-uniform
 *     branch), so one batch can mix stripes that rebuild one part with
 *     stripes that rebuild two.
 *
 * The index lookup reads through a const __restrict__ kernel argument at an
 * address derived from blockIdx only, so it is a scalar load like the
 * pointer-table reads.
 */
#pragma once
#include "ec_kernel.h"

template <int D, int CH, bool SWZ, bool NTST, bool NTLD>
__global__ __launch_bounds__(kThreads) void ec_encode_multi_kernel(
    uint32_t part_len, int srcs, int dest_base,
    const uint8_t *__restrict__ tables_dev,  /* [ntables][dests_total][srcs][32] */
    const uint32_t *__restrict__ tbl_index,  /* [stripes] */
    const uint64_t *__restrict__ src_ptrs,   /* [stripes][srcs]  */
    const uint64_t *__restrict__ dst_ptrs,   /* [stripes][dests_total]; 0 = skip */
    int dests_total, uint32_t tiles_per_part, uint32_t total_tiles) {
	constexpr uint32_t kTile = kChunkBytes * CH;
	constexpr uint32_t kNoTable = 0xffffffffu;
	extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
	const uint32_t tid = threadIdx.x;
	const size_t tbl_stride = (size_t)dests_total * srcs * 32;
	const int nbytes = D * srcs * 32;

	uint32_t staged = kNoTable;
	uint32_t b0 = SWZ ? xcd_remap(blockIdx.x, gridDim.x) : blockIdx.x;
	for (uint32_t tile = b0; tile < total_tiles; tile += gridDim.x) {
		uint32_t stripe = tile / tiles_per_part;
		uint32_t tin = tile - stripe * tiles_per_part;
		uint32_t base = tin * kTile + tid * 16u;
		const uint64_t *sp_tab = src_ptrs + (uint64_t)stripe * srcs;
		const uint64_t *dp_tab =
		    dst_ptrs + (uint64_t)stripe * dests_total + dest_base;

		/* Stage this tile's table rows: [D][srcs][32] bytes of table
		 * tbl_index[stripe].  Other waves may still be reading the rows
		 * of the previous tile, hence the barrier before the overwrite. */
		const uint32_t ti = tbl_index[stripe];
		if (ti != staged) {
			__syncthreads();
			const uint8_t *src_tbl = tables_dev + (size_t)ti * tbl_stride +
			                         (size_t)dest_base * srcs * 32;
			for (int i = tid * 16; i < nbytes; i += kThreads * 16)
				*(uint4 *)(smem + i) = *(const uint4 *)(src_tbl + i);
			__syncthreads();
			staged = ti;
		}

		uint4 acc[D][CH];
#pragma unroll
		for (int d = 0; d < D; ++d)
#pragma unroll
			for (int c = 0; c < CH; ++c)
				acc[d][c] = make_uint4(0, 0, 0, 0);

		auto tbl_read = [&](int j, uint4 (&Lb)[D], uint4 (&Hb)[D]) {
#pragma unroll
			for (int d = 0; d < D; ++d) {
				const uint8_t *tb = smem + ((size_t)d * srcs + j) * 32;
				Lb[d] = *(const uint4 *)tb;
				Hb[d].x = *(const uint32_t *)(tb + 16);
			}
		};

		if ((uint64_t)(tin + 1) * kTile <= part_len) {
			/* full tile: branchless; next source's strips prefetched
			 * while the current source is accumulated */
			uint4 w[CH], wn[CH];
			uint4 L[D], H[D];
			{
				const uint8_t *sp = (const uint8_t *)sp_tab[0];
#pragma unroll
				for (int c = 0; c < CH; ++c)
					w[c] = NTLD ? ld_nt(sp + (base + c * kChunkBytes))
					            : *(const uint4 *)(sp + (base + c * kChunkBytes));
			}
			auto step = [&](int j) {
				if (j + 1 < srcs) {
					const uint8_t *spn = (const uint8_t *)sp_tab[j + 1];
#pragma unroll
					for (int c = 0; c < CH; ++c)
						wn[c] = NTLD ? ld_nt(spn + (base + c * kChunkBytes))
						             : *(const uint4 *)(spn + (base + c * kChunkBytes));
				}
				tbl_read(j, L, H);
#pragma unroll
				for (int c = 0; c < CH; ++c)
					gf_macc_all_mr<D, CH>(acc, c, w[c], L, H);
#pragma unroll
				for (int c = 0; c < CH; ++c) w[c] = wn[c];
			};
			int j = 0;
			for (; j + 1 < srcs; j += 2) {
				step(j);
				step(j + 1);
			}
			if (j < srcs) step(j);
#pragma unroll
			for (int d = 0; d < D; ++d) {
				uint8_t *dp = (uint8_t *)dp_tab[d];
				if (dp == nullptr) continue;   /* wave-uniform */
#pragma unroll
				for (int c = 0; c < CH; ++c) {
					uint4 *p = (uint4 *)(dp + (base + c * kChunkBytes));
					if (NTST) {
						typedef unsigned int u32x4
						    __attribute__((ext_vector_type(4)));
						u32x4 v = {acc[d][c].x, acc[d][c].y, acc[d][c].z,
						           acc[d][c].w};
						__builtin_nontemporal_store(v, (u32x4 *)p);
					} else {
						*p = acc[d][c];
					}
				}
			}
		} else {
			/* ragged tail tile: per-strip bounds checks */
			for (int j = 0; j < srcs; ++j) {
				const uint8_t *sp = (const uint8_t *)sp_tab[j];
				uint4 L[D], H[D];
				tbl_read(j, L, H);
#pragma unroll
				for (int c = 0; c < CH; ++c) {
					uint32_t off = base + c * kChunkBytes;
					if (off < part_len) {
						uint4 w = *(const uint4 *)(sp + off);
						gf_macc_all_mr<D, CH>(acc, c, w, L, H);
					}
				}
			}
#pragma unroll
			for (int d = 0; d < D; ++d) {
				uint8_t *dp = (uint8_t *)dp_tab[d];
				if (dp == nullptr) continue;   /* wave-uniform */
#pragma unroll
				for (int c = 0; c < CH; ++c) {
					uint32_t off = base + c * kChunkBytes;
					if (off < part_len) *(uint4 *)(dp + off) = acc[d][c];
				}
			}
		}
	}
}
