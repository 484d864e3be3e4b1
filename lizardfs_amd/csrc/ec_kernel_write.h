/* ec_kernel_write.h — sibling of ec_chunk_read_kernel for the CLIENT WRITE:
 * the parity of byte ranges written into the chunk blocks of one slice, and
 * the CRC of every packet that leaves.
 *
 * This is ChunkWriter::startOperation (mount/chunk_writer.cc:475-547) with
 * computeParityBlock (:365-402) in one pass.  A write carries `size` new
 * bytes, the range [from, to) of a 64 KiB block, for each of the chunk
 * blocks [first, first + count); chunk block c is row c / ks, column c % ks
 * of the slice.  In every row b that the range touches, column c is
 *  - NEW   iff first <= b*ks + c < first + count: the caller's bytes at
 *          data + (b*ks + c - first) * data_stride;
 *  - FILL  else iff b < fill_nblocks[write][c]: bytes [from, to) of block b
 *          of the part behind the column, read back as fillStripe (:440-466)
 *          does, at fill[c] + b * fill_stride + from;
 *  - ABSENT otherwise (the zero padding past the chunk's end, :451): neither
 *          loaded nor addressed;
 * and parity r of the row is table row r over the columns, written at
 * par[r] + (b - r0) * par_stride, r0 the first touched row.  A parity whose
 * address is 0 is not wanted and not stored; a pass none of whose D
 * parities is wanted returns at once.
 *
 * Tile map (one entry per workgroup, built on the host), xcd_remap, LDS table
 * staging after the first loads are issued, pipelined accumulation through
 * gf_macc_all_mr and dest_base passes are those of ec_chunk_read_kernel.
 * What differs is the byte granularity.  Tiles are cut in range offsets
 * [0, size): tile t of a row holds n = min(kTile, size - t * kTile) bytes,
 * n16 = n & ~15 of them in whole 16-byte units that the lanes take (lane l,
 * strip c: unit at l*16 + c*4096, iff below n16) and n & 15 tail bytes
 * behind them that lanes 0..14 take one byte each.  Every source and every
 * destination has its own address mod 16, uniform over the workgroup, and
 * picks its form on that scalar:
 *   load   a = 0      one aligned 16-byte load
 *          a = 4q     one 16-byte load that promises 4-byte alignment
 *          other      that load 1..3 bytes down, at the dword boundary below,
 *                     plus the dword behind it, funnel-shifted
 *                     (v_alignbyte_b32) back into place
 *   store  d = 0      one aligned 16-byte store
 *          d = 4q     one 16-byte store that promises 4-byte alignment
 *          other      16 single bytes (crc_store_byte, crc_ranges.h)
 * No address is rounded down past the dword that holds the first byte and
 * no load reaches past the dword that holds the last: every aligned 16-byte
 * unit a load touches holds a byte of the range, and exactly the range's
 * bytes are stored.
 *
 * FAST is the form of a call in which every used address, every used
 * stride, every `from` and every size is a multiple of 16 (whole blocks into
 * aligned images): aligned loads and stores only, no form to pick, no tail.
 *
 * Every branch but the per-lane "my unit lies below n16" / "my tail byte
 * exists" predicates compares scalars loaded at workgroup-uniform addresses.
 * Sources and destinations come out of tables, so they are cast to address
 * space 1 by hand (global, not flat, accesses; crc_ranges.h).
 */
#pragma once
#include "../../include/lizec.h"
#include "crc_ranges.h"
#include "ec_kernel_read.h"

typedef const __attribute__((address_space(1))) ec_u32x4 *ecw_ld_a16;
typedef const __attribute__((address_space(1))) ec_u32x4_a4 *ecw_ld_a4;
typedef const __attribute__((address_space(1))) uint32_t *ecw_ld_w;
typedef __attribute__((address_space(1))) ec_u32x4 *ecw_st_a16;
typedef __attribute__((address_space(1))) ec_u32x4_a4 *ecw_st_a4;

/* Issue the loads of one column's units: lane unit c lies at src + lane_off +
 * c * 4096 and is loaded iff it ends at or below n16.  `a` = src mod 16.
 * Unaligned forms leave w raw (loaded a & 3 bytes down) with the dword
 * behind it in e; ecw_fix puts the bytes in place. */
template <int CH, bool FAST>
__device__ __forceinline__ void ecw_issue(uint64_t src, uint32_t lane_off,
                                          uint32_t n16, uint4 (&w)[CH],
                                          uint32_t (&e)[CH]) {
	const uint32_t a = (uint32_t)src & 15u;
	if (FAST || a == 0) {
#pragma unroll
		for (int c = 0; c < CH; ++c) {
			const uint32_t o = lane_off + c * kChunkBytes;
			if (o < n16) {
				ec_u32x4 v = __builtin_nontemporal_load((ecw_ld_a16)(src + o));
				w[c] = make_uint4(v.x, v.y, v.z, v.w);
			}
		}
	} else {
		const uint32_t r = a & 3u;
		const uint64_t down = src - r;
#pragma unroll
		for (int c = 0; c < CH; ++c) {
			const uint32_t o = lane_off + c * kChunkBytes;
			if (o < n16) {
				ec_u32x4 v = __builtin_nontemporal_load((ecw_ld_a4)(down + o));
				w[c] = make_uint4(v.x, v.y, v.z, v.w);
				/* r = 0: the dword behind may lie outside the range */
				if (r) e[c] = __builtin_nontemporal_load(
				           (ecw_ld_w)(down + o + 16));
			}
		}
	}
}

/* Shift the units of a column loaded r = src & 3 bytes down into place. */
template <int CH>
__device__ __forceinline__ void ecw_fix(uint32_t r, uint4 (&w)[CH],
                                        const uint32_t (&e)[CH]) {
	if (r == 0) return;
#pragma unroll
	for (int c = 0; c < CH; ++c) {
		w[c].x = __builtin_amdgcn_alignbyte(w[c].y, w[c].x, r);
		w[c].y = __builtin_amdgcn_alignbyte(w[c].z, w[c].y, r);
		w[c].z = __builtin_amdgcn_alignbyte(w[c].w, w[c].z, r);
		w[c].w = __builtin_amdgcn_alignbyte(e[c], w[c].w, r);
	}
}

/* Store one parity's units of the tile at dst (the tile's first byte). */
template <int CH, bool FAST>
__device__ __forceinline__ void ecw_store(uint64_t dst, uint32_t lane_off,
                                          uint32_t n16,
                                          const uint4 (&acc)[CH]) {
	const uint32_t d = (uint32_t)dst & 15u;
	if (FAST || (d & 3u) == 0) {
#pragma unroll
		for (int c = 0; c < CH; ++c) {
			const uint32_t o = lane_off + c * kChunkBytes;
			if (o < n16) {
				ec_u32x4 v = {acc[c].x, acc[c].y, acc[c].z, acc[c].w};
				if (FAST || d == 0)
					__builtin_nontemporal_store(v, (ecw_st_a16)(dst + o));
				else
					__builtin_nontemporal_store(v, (ecw_st_a4)(dst + o));
			}
		}
	} else {
#pragma unroll
		for (int c = 0; c < CH; ++c) {
			const uint32_t o = lane_off + c * kChunkBytes;
			if (o < n16) {
				const crc_gbytes_w b = (crc_gbytes_w)(dst + o);
				const uint32_t ws[4] = {acc[c].x, acc[c].y, acc[c].z,
				                        acc[c].w};
#pragma unroll
				for (int k = 0; k < 16; ++k)
					crc_store_byte(b + k, ws[k >> 2] >> (8 * (k & 3)));
			}
		}
	}
}

template <int D, int CH, bool FAST>
__global__ __launch_bounds__(kThreads) void ec_chunk_write_kernel(
    int ks, int dest_base, int rows_total,
    const uint8_t *__restrict__ tables_dev,      /* [rows_total][ks][32] */
    const uint4 *__restrict__ tile_map,          /* [gridDim.x]: write, row,
                                                    tile, row - first row */
    const lizec_chunk_write *__restrict__ writes,
    const uint64_t *__restrict__ fill_ptrs,      /* [writes][ks] */
    const uint32_t *__restrict__ fill_nblocks,   /* [writes][ks] */
    const uint64_t *__restrict__ par_ptrs,       /* [writes][rows_total] */
    uint32_t fill_stride) {
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

	/* column c of this row: the tile's first byte, or 0 = absent */
	const uint64_t *fp_tab = fill_ptrs + (uint64_t)wi * ks;
	const uint32_t *fn_tab = fill_nblocks + (uint64_t)wi * ks;
	const uint32_t c0 = blk * (uint32_t)ks;
	auto source = [&](int c) -> uint64_t {
		const uint32_t i = c0 + (uint32_t)c - wr.first_block;   /* wraps */
		if (i < wr.block_count)
			return wr.data + (i ? (uint64_t)i * wr.data_stride : 0) + off0;
		if (blk < fn_tab[c])
			return fp_tab[c] + (uint64_t)blk * fill_stride + wr.from + off0;
		return 0;
	};
	const uint32_t lane_off = tid * 16u;

	uint4 acc[D][CH];
#pragma unroll
	for (int d = 0; d < D; ++d)
#pragma unroll
		for (int c = 0; c < CH; ++c)
			acc[d][c] = make_uint4(0, 0, 0, 0);

	uint4 w[CH], wn[CH];
	uint32_t e[CH], en[CH];
	uint4 T[D], T6[D];
#pragma unroll
	for (int c = 0; c < CH; ++c) {
		w[c] = wn[c] = make_uint4(0, 0, 0, 0);
		e[c] = en[c] = 0;
	}
	/* cur: the column whose units are in w (0 = absent) */
	uint64_t cur = source(0);
	if (cur) ecw_issue<CH, FAST>(cur, lane_off, n16, w, e);
	/* stage this pass's rows of the table: [D][ks][32] bytes, after the
	 * first loads are issued (ec_kernel_ragged.h) */
	{
		const uint8_t *src_tbl = tables_dev + (size_t)dest_base * ks * 32;
		int nbytes = D * ks * 32;
		for (int i = tid * 16; i < nbytes; i += kThreads * 16)
			*(uint4 *)(smem + i) = *(const uint4 *)(src_tbl + i);
		__syncthreads();
	}
	/* one column step: accumulate column j while column j+1's units (if it
	 * has any) are in flight */
	auto step = [&](int j) {
		uint64_t nxt = 0;
		if (j + 1 < ks) {
			nxt = source(j + 1);
			if (nxt) ecw_issue<CH, FAST>(nxt, lane_off, n16, wn, en);
		}
		if (cur) {
			if (!FAST) ecw_fix<CH>((uint32_t)cur & 3u, w, e);
#pragma unroll
			for (int d = 0; d < D; ++d) {
				const uint8_t *tb = smem + ((size_t)d * ks + j) * 32;
				T[d] = *(const uint4 *)tb;
				T6[d].x = *(const uint32_t *)(tb + 16);
			}
#pragma unroll
			for (int c = 0; c < CH; ++c)
				gf_macc_all_mr<D, CH>(acc, c, w[c], T, T6);
		}
#pragma unroll
		for (int c = 0; c < CH; ++c) {
			w[c] = wn[c];
			e[c] = en[c];
		}
		cur = nxt;
	};
	int j = 0;
	for (; j + 1 < ks; j += 2) {
		step(j);
		step(j + 1);
	}
	if (j < ks) step(j);
#pragma unroll
	for (int d = 0; d < D; ++d) {
		if (!dst[d]) continue;   /* workgroup-uniform */
		ecw_store<CH, FAST>(dst[d], lane_off, n16, acc[d]);
	}
	if (!FAST) {
		/* the bytes behind the last whole unit: lane i takes byte n16 + i
		 * through every column, one table product per parity */
		if (tail) {
			const bool mine = tid < tail;
			const uint32_t at = n16 + tid;
			uint32_t a1[D];
#pragma unroll
			for (int d = 0; d < D; ++d) a1[d] = 0;
			for (int c = 0; c < ks; ++c) {
				const uint64_t s = source(c);
				if (!s) continue;
				uint32_t b = 0;
				if (mine) b = *(crc_gbytes)(s + at);
				const uint32_t f0 = b & 7u, f1 = (b >> 3) & 7u, f2 = b >> 6;
#pragma unroll
				for (int d = 0; d < D; ++d) {
					const uint8_t *tb = smem + ((size_t)d * ks + c) * 32;
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

/* The packets' CRCs are computed by crc32_ranges_kernel (crc_ranges.h) over
 * the data and parity ranges, behind the parity passes on the same stream,
 * into the call's scratch; this moves them to the slots of the writes' own
 * CRC arrays: *outs[i] = crcs[i], one thread per CRC. */
__global__ __launch_bounds__(kCrcRangesThreads) void chunk_write_crc_scatter_kernel(
    const uint32_t *__restrict__ crcs, const uint64_t *__restrict__ outs,
    uint32_t n) {
	const uint32_t i = blockIdx.x * kCrcRangesThreads + threadIdx.x;
	if (i < n) *(uint32_t *)outs[i] = crcs[i];
}
