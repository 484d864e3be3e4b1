/* ec_kernel_strided.h — ec_encode_kernel for parts stored as 64 KiB blocks
 * at a fixed stride, at addresses that are only 4-byte aligned.
 *
 * This is the layout of an INTERLEAVED-format chunk part (chunk.h:40
 * kHddBlockSize = 65540, chunk.cc:191-209): every block is preceded by its
 * own 4-byte CRC, so block b's data starts at 4 + 65540*b and its alignment
 * cycles through 4, 8, 12, 0 mod 16.  A part here is `nblocks` blocks of
 * 65536 bytes, block b at ptr + b*stride; sources and destinations have a
 * stride each.
 *
 * Same arithmetic, LDS table staging, XCD remap and 1 KiB-per-wave access
 * pattern as ec_encode_kernel (ec_kernel.h), with three differences:
 *  - both tile sizes (16 KiB, 8 KiB) divide 65536, so a tile lies inside
 *    one block and every tile is full: only the pipelined branchless body
 *    exists, and the block's offset is one 64-bit scalar per tile;
 *  - one tile per workgroup, no grid-stride loop (the host launches
 *    exactly total_tiles workgroups and refuses larger batches);
 *  - SAL / DAL say whether the source / destination side is 16-byte
 *    aligned (every pointer and the stride).  An unaligned side still moves
 *    16 bytes per lane, through a vector type that promises only 4-byte
 *    alignment; it never rounds an address down, so no byte outside
 *    [block, block + 65536) is read or written and the bytes between two
 *    destination blocks (the CRC slots) survive.
 */
#pragma once
#include "ec_kernel.h"

constexpr uint32_t kECBlockBytes = 65536;   /* MFSBLOCKSIZE */

typedef unsigned int ec_u32x4 __attribute__((ext_vector_type(4)));
typedef ec_u32x4 ec_u32x4_a4 __attribute__((aligned(4)));

/* non-temporal 16-byte load / store; AL16=false for addresses that are
 * only 4-byte aligned */
template <bool AL16>
__device__ __forceinline__ uint4 ec_ld16(const uint8_t *p) {
	if constexpr (AL16) {
		return ld_nt(p);
	} else {
		ec_u32x4 v = __builtin_nontemporal_load((const ec_u32x4_a4 *)p);
		return make_uint4(v.x, v.y, v.z, v.w);
	}
}

template <bool AL16>
__device__ __forceinline__ void ec_st16(uint8_t *p, const uint4 &a) {
	ec_u32x4 v = {a.x, a.y, a.z, a.w};
	if constexpr (AL16)
		__builtin_nontemporal_store(v, (ec_u32x4 *)p);
	else
		__builtin_nontemporal_store(v, (ec_u32x4_a4 *)p);
}

template <int D, int CH, bool SAL, bool DAL>
__global__ __launch_bounds__(kThreads) void ec_encode_strided_kernel(
    uint32_t tiles_per_part,                 /* nblocks * tiles per block */
    int srcs, int dest_base,
    const uint8_t *__restrict__ gftbls_dev,  /* 32*srcs*dests_total, packed */
    const uint64_t *__restrict__ src_ptrs,   /* [stripes][srcs]  */
    const uint64_t *__restrict__ dst_ptrs,   /* [stripes][dests_total] */
    int dests_total, uint32_t src_stride, uint32_t dst_stride) {
	constexpr uint32_t kTile = kChunkBytes * CH;
	static_assert(kECBlockBytes % kTile == 0, "a tile must not straddle");
	constexpr uint32_t kTilesPerBlock = kECBlockBytes / kTile;
	extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
	const uint32_t tid = threadIdx.x;

	/* stage this pass's table rows: [D][srcs][32] bytes, mixed-radix */
	{
		const uint8_t *src_tbl = gftbls_dev + (size_t)dest_base * srcs * 32;
		int nbytes = D * srcs * 32;
		for (int i = tid * 16; i < nbytes; i += kThreads * 16)
			*(uint4 *)(smem + i) = *(const uint4 *)(src_tbl + i);
	}
	__syncthreads();

	/* tile -> (stripe, block, tile in block); gridDim.x == total tiles */
	const uint32_t tile = xcd_remap(blockIdx.x, gridDim.x);
	const uint32_t stripe = tile / tiles_per_part;
	const uint32_t tin = tile - stripe * tiles_per_part;
	const uint32_t blk = tin / kTilesPerBlock;
	const uint32_t in_blk = (tin % kTilesPerBlock) * kTile;
	/* workgroup-uniform 64-bit block offsets, per-lane 32-bit remainder */
	const uint64_t soff = (uint64_t)blk * src_stride + in_blk;
	const uint64_t doff = (uint64_t)blk * dst_stride + in_blk;
	const uint32_t lane_off = tid * 16u;
	const uint64_t *sp_tab = src_ptrs + (uint64_t)stripe * srcs;
	const uint64_t *dp_tab =
	    dst_ptrs + (uint64_t)stripe * dests_total + dest_base;

	uint4 acc[D][CH];
#pragma unroll
	for (int d = 0; d < D; ++d)
#pragma unroll
		for (int c = 0; c < CH; ++c)
			acc[d][c] = make_uint4(0, 0, 0, 0);

	uint4 w[CH], wn[CH];
	uint4 T[D], T6[D];
	{
		const uint8_t *sp = (const uint8_t *)sp_tab[0] + soff;
#pragma unroll
		for (int c = 0; c < CH; ++c)
			w[c] = ec_ld16<SAL>(sp + (lane_off + c * kChunkBytes));
	}
	/* one source step: accumulate source j while source j+1's strips are
	 * in flight */
	auto step = [&](int j) {
		if (j + 1 < srcs) {
			const uint8_t *spn = (const uint8_t *)sp_tab[j + 1] + soff;
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
	int j = 0;
	for (; j + 1 < srcs; j += 2) {
		step(j);
		step(j + 1);
	}
	if (j < srcs) step(j);
#pragma unroll
	for (int d = 0; d < D; ++d) {
		uint8_t *dp = (uint8_t *)dp_tab[d] + doff;
#pragma unroll
		for (int c = 0; c < CH; ++c)
			ec_st16<DAL>(dp + (lane_off + c * kChunkBytes), acc[d][c]);
	}
}
