/* crc_ranges.h — CRC32 of independent byte ranges of any length and any
 * alignment, and the batched hdd_write gate built on it.
 *
 * The block kernels (crc_fold.h) want whole, equal, 4-byte-aligned blocks.
 * hdd_write (hddspacemgr.cc:1899-2009) hashes whatever the client sends —
 * `size` bytes at `offset` inside a 64 KiB block — and, for a partial write,
 * the three byte ranges around it.  Here one wave owns one range
 * [addr, addr + len), len <= 65536, and cuts it into
 *
 *   head   the bytes before the first 16-byte boundary (0..15), walked by
 *          lane 0 from the seed,
 *   body   U whole 16-byte units, aligned, dealt out to the lanes as
 *          contiguous runs of Q = ceil(U / 64) units FROM THE END: lane 63
 *          holds the last Q, lane 62 the Q before them, and so on; the
 *          first lane that still gets units holds what is left (1..Q),
 *          lanes before it hold none,
 *   tail   the bytes behind the last whole unit (0..15), walked after the
 *          lanes are combined.
 *
 * Head and tail go through the byte table T0 with single-byte loads, the
 * body through aligned 16-byte loads: no byte outside the range is read.
 *
 * Table bytes versus 16-byte folds.  A lane's units all go through the
 * 128-bit fold (crc_fold16, pure VALU), the running state XORed into the
 * first, and the accumulator is reduced once with 16 table steps
 * (crc_reduce16).  For exactly one unit that IS the 16 table steps a
 * bytewise walk would take, so folding costs nothing extra from the first
 * unit on and saves 16 lookups for each further one: the switch point is
 * one whole aligned unit.  Only head and tail bytes, and ranges too short
 * to hold an aligned unit, are pure table work.
 *
 * One instantiation serves every length.  A lane's run is folded in bursts
 * of 8, then 4, 2 and 1 units (loads of a burst issued together), so a
 * 64 KiB range is 8 bursts of 8 per lane, a 4 KiB range one burst of 4 and
 * a 1 KiB range one unit per lane.  Below 1 KiB lanes idle; a second
 * instantiation that puts several short ranges into one wave would use
 * them, but every range would still pay the combine below, and the write
 * path's ranges are KiB-sized — not built (profiles/CRC_RANGES.md has the
 * measured short-range rate).
 *
 * Combining the lanes.  The block kernels fold per-lane CRCs in a shfl tree
 * that appends, at step s, the run of the 2^s lanes to the right: equal
 * runs make that ONE matrix per step, the same for all lanes.  With runs
 * of unequal length every lane asks for a different zero run, crc_advance's
 * loop runs over the union of their set bits, six times over, and 4 KiB
 * ranges at odd addresses ran at 0.36 TB/s (profiles/CRC_RANGES.md, first
 * form).  So the lanes are combined flat, in
 * the un-inverted ("raw") domain where the CRC register is linear in the
 * message: lane 0 starts from seed ^ ~0, every other lane from 0; lane l
 * advances its end state by the k_l = min(U, Q * (63 - l)) units that
 * follow its run (crc_advance, 16 * k_l bytes) and the 64 results are
 * XORed.  Dealing the units from the end makes k_l a multiple of Q with no
 * remainder term, so the union of set bits stays at 6 positions plus those
 * of Q whatever the alignment.  A lane that holds nothing still has raw
 * state 0, advance(0, n) = 0, and XOR drops it: the empty-lane case of the
 * tree (advance(c, 0) ^ 0 = c) has no counterpart to get wrong here.  Lane
 * 0 may hold head bytes and no unit; its k is then U.  The tail bytes are
 * walked from the combined state, and the result is inverted once.
 *
 * The range addresses come out of a table, so the compiler cannot tell that
 * they are global memory; they are cast to address space 1 by hand, which
 * turns flat loads (counted against the LDS queue too) into global loads.
 *
 * LDS holds the constants only (T0 and the advance matrices M_0..M_16,
 * enough for zero runs up to 2^17 - 1 bytes), as in the fold kernels.
 *
 * The walk can carry a copy of the range (COPY; the read gate, read_gate.h):
 * what it loads it also stores, shifted by a fixed distance.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/lizec.h"
#include "crc_fold.h"

constexpr int kCrcRangesThreads = 256;            /* 4 waves, one range each */
constexpr int kCrcRangesMats = 17;                /* M_0..M_16: runs < 2^17 */
constexpr int kCrcRangesLdsWords = 256 + kCrcRangesMats * 32;
constexpr uint32_t kCrcRangeMaxLen = 65536u;      /* MFSBLOCKSIZE */

typedef unsigned int crc_u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) crc_u32x4 *crc_gunits;
typedef const __attribute__((address_space(1))) uint8_t *crc_gbytes;

/* The copy a range pass can carry (the read gate, read_gate.h): the bytes
 * of the range are stored at `dst + (their offset in the range)` as they
 * are walked.  The source units are 16-byte aligned; what their copies are
 * aligned to is wave-uniform and picks the store: 16 bytes, a 16-byte
 * vector that promises 4-byte alignment only (as ec_kernel_strided.h
 * does), or 16 single bytes.  kCrcCopyNone walks without storing. */
enum : uint32_t { kCrcCopy16 = 0, kCrcCopy4 = 1, kCrcCopy1 = 2,
                  kCrcCopyNone = 3 };
typedef crc_u32x4 crc_u32x4_a4 __attribute__((aligned(4)));
typedef __attribute__((address_space(1))) crc_u32x4 *crc_gunits_w;
typedef __attribute__((address_space(1))) crc_u32x4_a4 *crc_gunits_w4;
typedef __attribute__((address_space(1))) uint8_t *crc_gbytes_w;

/* form = (dst - src) mod 16 of a copy, as a store form */
__device__ __forceinline__ uint32_t crc_copy_form(uint64_t dst, uint64_t src) {
	const uint32_t d = (uint32_t)(dst - src) & 15u;
	return d == 0 ? kCrcCopy16 : (d & 3u) == 0 ? kCrcCopy4 : kCrcCopy1;
}

/* One byte, stored as one byte.  Plain neighbouring byte stores are merged
 * by the compiler into dword and 16-byte stores at whatever address they
 * have; a relaxed atomic of wavefront scope is the same global_store_byte,
 * with no cache bits and no wait, and is left alone. */
__device__ __forceinline__ void crc_store_byte(crc_gbytes_w p, uint32_t v) {
	__hip_atomic_store(p, (uint8_t)v, __ATOMIC_RELAXED,
	                   __HIP_MEMORY_SCOPE_WAVEFRONT);
}

/* Store one 16-byte unit at dst in the given form (not kCrcCopyNone). */
__device__ __forceinline__ void crc_store_unit(uint64_t dst, uint32_t form,
                                               crc_u32x4 w) {
	if (form == kCrcCopy16) {
		*(crc_gunits_w)dst = w;
	} else if (form == kCrcCopy4) {
		*(crc_gunits_w4)dst = w;
	} else {
		const crc_gbytes_w b = (crc_gbytes_w)dst;
#pragma unroll
		for (int k = 0; k < 16; ++k)
			crc_store_byte(b + k, w[k >> 2] >> (8 * (k & 3)));
	}
}

/* Fold units [i, i + N) of a lane's run into acc: N loads, then N folds.
 * The lane's incoming state `s` goes into the first word of unit 0; the
 * accumulator starts as zero there, and folding zero leaves the data.
 * With COPY the units are stored at dst + 16 * (i + q) as loaded. */
template <int N, bool OR, bool COPY = false>
__device__ __forceinline__ void crc_range_burst(uint32_t (&acc)[4],
                                                crc_gunits u, uint32_t i,
                                                uint32_t s, uint32_t &nz,
                                                uint64_t dst = 0,
                                                uint32_t form = kCrcCopyNone) {
	crc_u32x4 w[N];
#pragma unroll
	for (int q = 0; q < N; ++q) w[q] = u[i + q];
	if (OR) {
#pragma unroll
		for (int q = 0; q < N; ++q) nz |= w[q].x | w[q].y | w[q].z | w[q].w;
	}
	if (COPY) {
		if (form != kCrcCopyNone) {
#pragma unroll
			for (int q = 0; q < N; ++q)
				crc_store_unit(dst + ((uint64_t)(i + q) << 4), form, w[q]);
		}
	}
	w[0].x ^= (i == 0 ? s : 0u);
#pragma unroll
	for (int q = 0; q < N; ++q)
		crc_fold16<kCrcFoldKL1, kCrcFoldKH1>(acc, w[q].x, w[q].y, w[q].z,
		                                     w[q].w);
}

/* Per-wave CRC of [p, p + len); p and len are wave-uniform.  Every lane
 * returns the CRC.  With OR, *any_nz tells whether any byte of the range is
 * non-zero.  With COPY and a form other than kCrcCopyNone the range is also
 * copied to [dst, dst + len): units by the lanes that fold them, head and
 * tail bytes by lane 0; form must be crc_copy_form(dst, addr). */
template <bool OR, bool COPY = false>
__device__ uint32_t crc_range_wave(uint64_t addr, uint32_t len, uint32_t seed,
                                   const uint32_t *T0, const uint32_t *mats,
                                   int lane, bool *any_nz, uint64_t dst = 0,
                                   uint32_t form = kCrcCopyNone) {
	const crc_gbytes p = (crc_gbytes)addr;
	const uint32_t to16 = (0u - (uint32_t)addr) & 15u;
	const uint32_t head = to16 < len ? to16 : len;
	const uint32_t units = (len - head) >> 4;
	const uint32_t tail = (len - head) & 15u;
	const uint32_t Q = (units + 63u) >> 6;
	/* lane l's run is units [first, end): Q-unit runs dealt from the end */
	const uint32_t after = Q * (uint32_t)(63 - lane);   /* k_l, unclamped */
	const uint32_t end = units > after ? units - after : 0u;
	const uint32_t first = end > Q ? end - Q : 0u;
	const uint32_t cnt = end - first;
	uint32_t s = lane == 0 ? seed ^ 0xFFFFFFFFu : 0u;    /* raw state */
	uint32_t nz = 0;
	if (lane == 0) {
		for (uint32_t i = 0; i < head; ++i) {
			uint32_t b = p[i];
			if (OR) nz |= b;
			if (COPY) {
				if (form != kCrcCopyNone) ((crc_gbytes_w)dst)[i] = (uint8_t)b;
			}
			s = (s >> 8) ^ T0[(s ^ b) & 0xFFu];
		}
	}
	if (cnt) {
		/* 16-byte aligned: addr + head is, whenever units > 0 */
		const crc_gunits u = (crc_gunits)(addr + head) + first;
		/* where this lane's unit 0 goes */
		const uint64_t d = dst + head + ((uint64_t)first << 4);
		uint32_t acc[4] = {0u, 0u, 0u, 0u};
		uint32_t i = 0;
		for (; i + 8 <= cnt; i += 8)
			crc_range_burst<8, OR, COPY>(acc, u, i, s, nz, d, form);
		if (i + 4 <= cnt) {
			crc_range_burst<4, OR, COPY>(acc, u, i, s, nz, d, form);
			i += 4;
		}
		if (i + 2 <= cnt) {
			crc_range_burst<2, OR, COPY>(acc, u, i, s, nz, d, form);
			i += 2;
		}
		if (i < cnt) crc_range_burst<1, OR, COPY>(acc, u, i, s, nz, d, form);
		s = crc_reduce16(acc, T0);
	}
	/* raw states are linear in the message: advance each lane's by the
	 * units behind its run and XOR them all */
	s = crc_advance(s, (units - end) << 4, mats);
#pragma unroll
	for (int m = 1; m < 64; m <<= 1) s ^= __shfl_xor(s, m, 64);
	/* The tail, from the combined state.  Unlike the head, which only lane
	 * 0 walks because only lane 0 carries the seed, the tail is walked by
	 * every lane: after the XOR above all 64 hold the same state, every
	 * lane has to return the final value, and `tail` is wave-uniform, so
	 * the loop needs no branch on the lane; the 64 loads of a step have one
	 * address and are served as one broadcast.  The bytes' OR comes out
	 * the same in every lane, which the ballot below does not mind. */
	const crc_gbytes t = p + head + (units << 4);
	for (uint32_t i = 0; i < tail; ++i) {
		uint32_t b = t[i];
		if (OR) nz |= b;
		if (COPY) {
			if (form != kCrcCopyNone && lane == 0)
				((crc_gbytes_w)dst)[head + (units << 4) + i] = (uint8_t)b;
		}
		s = (s >> 8) ^ T0[(s ^ b) & 0xFFu];
	}
	if (OR) *any_nz = __ballot(nz != 0) != 0;
	return s ^ 0xFFFFFFFFu;
}

/* out[i] = crc32(seed, addrs[i], lens[i]); one wave per range, grid
 * stride, the next range's table entry loaded while this one is hashed.
 * With OR, nz_out[i] = 1 if the range holds a non-zero byte. */
template <bool OR>
__global__ __launch_bounds__(kCrcRangesThreads) void crc32_ranges_kernel(
    const uint64_t *__restrict__ addrs, const uint32_t *__restrict__ lens,
    uint32_t n, uint32_t seed, const uint32_t *__restrict__ tab0,
    const uint32_t *__restrict__ mats_g, uint32_t *__restrict__ out,
    uint32_t *__restrict__ nz_out) {
	__shared__ __attribute__((aligned(16))) uint32_t stabs[kCrcRangesLdsWords];
	const uint32_t wave = threadIdx.x >> 6;
	const int lane = threadIdx.x & 63;
	const uint32_t stride = gridDim.x * 4;
	uint32_t i = blockIdx.x * 4 + wave;
	uint64_t addr = 0;
	uint32_t len = 0;
	if (i < n) {
		addr = addrs[i];
		len = lens[i];
	}
	for (int k = threadIdx.x; k < 256; k += kCrcRangesThreads)
		stabs[k] = tab0[k];
	for (int k = threadIdx.x; k < kCrcRangesMats * 32; k += kCrcRangesThreads)
		stabs[256 + k] = mats_g[k];
	__syncthreads();
	while (i < n) {
		/* n <= 2^26 and stride <= 2^16: no wrap */
		const uint32_t nx = i + stride;
		uint64_t naddr = 0;
		uint32_t nlen = 0;
		if (nx < n) {
			naddr = addrs[nx];
			nlen = lens[nx];
		}
		bool any = false;
		uint32_t crc = crc_range_wave<OR>(addr, len, seed, stabs, stabs + 256,
		                                  lane, &any);
		if (lane == 0) {
			out[i] = crc;
			if (OR) nz_out[i] = any ? 1u : 0u;
		}
		i = nx;
		addr = naddr;
		len = nlen;
	}
}

/* mycrc32_zeroblock(0, zeros) (crc.h:27) on the matrix bank. */
__device__ __forceinline__ uint32_t crc_zeroblock0(uint32_t zeros,
                                                   const uint32_t *mats) {
	return crc_advance(0xFFFFFFFFu, zeros, mats) ^ 0xFFFFFFFFu;
}

/* hdd_write's recombine (hddspacemgr.cc:1954-1962 and :1992-1999), the
 * device twin of lizec_crc32_splice at block_len 65536. */
__device__ __forceinline__ uint32_t crc_splice64k(uint32_t pre,
                                                  uint32_t offset,
                                                  uint32_t crc, uint32_t size,
                                                  uint32_t post,
                                                  const uint32_t *mats) {
	const uint32_t rest = 65536u - (offset + size);
	if (offset == 0) return crc_advance(crc, rest, mats) ^ post;
	uint32_t c = crc_advance(pre, size, mats) ^ crc;
	if (rest) c = crc_advance(c, rest, mats) ^ post;
	return c;
}

/* The gate's finishing step, one thread per op.  crcs / nz hold four slots
 * per op from the ranges pass: [data, pre, changed, post] (a slot the op
 * does not need has length 0).  Writes status[i] and newcrc[i] only. */
__global__ __launch_bounds__(kCrcRangesThreads) void write_gate_finish_kernel(
    const lizec_write_op *__restrict__ ops, uint32_t n, uint32_t flags,
    const uint32_t *__restrict__ crcs, const uint32_t *__restrict__ nz,
    const uint32_t *__restrict__ mats_g, int32_t *__restrict__ status,
    uint32_t *__restrict__ newcrc) {
	__shared__ uint32_t mats[kCrcRangesMats * 32];
	for (int i = threadIdx.x; i < kCrcRangesMats * 32; i += kCrcRangesThreads)
		mats[i] = mats_g[i];
	__syncthreads();
	const uint32_t i = blockIdx.x * kCrcRangesThreads + threadIdx.x;
	if (i >= n) return;
	const lizec_write_op op = ops[i];
	int32_t st = LIZEC_GATE_OK;
	uint32_t out = 0;
	if (op.crc != crcs[4 * i]) {
		st = LIZEC_GATE_BAD_DATA;
	} else if (op.offset == 0 && op.size == 65536u) {
		out = op.crc;
	} else {
		const uint32_t rest = 65536u - (op.offset + op.size);
		uint32_t pre, post;
		if (op.block == 0) {
			pre = crc_zeroblock0(op.offset, mats);
			post = crc_zeroblock0(rest, mats);
		} else {
			pre = crcs[4 * i + 1];
			post = crcs[4 * i + 3];
			const uint32_t have = crc_splice64k(pre, op.offset, crcs[4 * i + 2],
			                                    op.size, post, mats);
			const uint8_t *p = (const uint8_t *)op.stored;
			uint32_t stored = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) |
			                  ((uint32_t)p[2] << 8) | p[3];
			if ((flags & LIZEC_GATE_SPARSE) && stored == 0 &&
			    (nz[4 * i + 1] | nz[4 * i + 2] | nz[4 * i + 3]) == 0)
				stored = crc_zeroblock0(65536u, mats);
			if (stored != have) st = LIZEC_GATE_BAD_BLOCK;
		}
		if (st == LIZEC_GATE_OK)
			out = crc_splice64k(pre, op.offset, op.crc, op.size, post, mats);
	}
	status[i] = st;
	newcrc[i] = out;
}
