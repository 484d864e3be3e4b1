/* lizec_gpu.hip — MI355X (gfx950/CDNA4) kernels + batch engine for the
 * LizardFS EC hot path.
 *
 * Replaces the reference's SIMD byte loop (galois_field_encode.cc:151-201,
 * AVX2 pshufb) with a CDNA4-native design:
 *  - GF(2^8) multiply via in-register mixed-radix (3+3+2 bit field)
 *    product LUTs selected with v_perm_b32 (__builtin_amdgcn_perm):
 *    3 perms + 3 XORs per destination word, tables re-read per tile as
 *    wave-uniform LDS broadcasts (ec_kernel.h gf_macc_mr);
 *  - 16-byte vectorized HBM loads/stores laid out so every wave instruction
 *    is a fully-coalesced 1 KiB access; full tiles run a branchless
 *    software-pipelined path (next source's strips prefetched while the
 *    current one is accumulated), ragged tails take a guarded path;
 *  - per-64KiB-block CRC32 (hddspacemgr.cc:1918 gate) with one wave per
 *    block via LDS-free carry-less folding (crc_fold.h) and a shfl-based
 *    combine tree using the same GF(2) "advance by N zero bytes" matrices
 *    as mycrc32_combine (crc.cc:153-224); slicing-table kernels remain
 *    for odd block sizes.
 *
 * This file is the product compute path: it REQUIRES a GPU.  There is no
 * CPU fallback here by design (parity claims are void otherwise).
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <atomic>
#include <mutex>
#include <unordered_map>

#include "../../include/lizec.h"

#define LIZEC_CHECK(x)                                                   \
	do {                                                                 \
		hipError_t _e = (x);                                             \
		if (_e != hipSuccess) return LIZEC_EHIP;                         \
	} while (0)

#include "ec_kernel.h"
#include "ec_kernel_multi.h"
#include "ec_kernel_strided.h"
#include "ec_kernel_ragged.h"
#include "ec_kernel_view.h"
#include "ec_kernel_read.h"
#include "crc_fold.h"
#include "crc_ranges.h"
#include "read_gate.h"
#include "read_verify.h"
#include "replicate_stage.h"
#include "ec_kernel_write.h"
#include "ec_kernel_write_degraded.h"

/* Product kernel configuration (chosen by the variant A/B harness,
 * bench_variants.hip; numbers in profiles/ROUND1.md + ROUND2.md):
 *  - XCD-bijective block remap + non-temporal parity stores everywhere;
 *  - tile size per destination-group width D: D<=2 uses 4-chunk (16 KiB)
 *    tiles; D>=3 uses 2-chunk (8 KiB) tiles (fewer accumulator VGPRs ->
 *    4 waves/SIMD; ec(16,4) D4: 3953 -> 4113 GB/s, ec(32,6) D6: 3001);
 *  - mixed-radix (3+3+2) GF tables: 3 v_perms + 3 XORs per dest word
 *    instead of the quarter-LUT's 4+4 — r2a/r2b A/B: ec(16,4) 4446 ->
 *    5392 GB/s (+21%), ec(32,6) 3239 -> 3953 (+22%), ec(8,2) tie. */
constexpr bool kECSwz = true;
constexpr bool kECNtStore = true;
constexpr bool kECNtLoad = true;   /* +3.6%: 5720 -> 5924 GB/s (profiles) */
constexpr int ec_chunks_for(int d) { return d <= 4 ? 4 : 2; }
constexpr int kECTblBytes = 32;    /* mixed-radix padded layout */

/* repack one 32-byte ISA-L coefficient table into the padded 32-byte
 * mixed-radix layout the MR kernel stages (see gf_macc_mr in ec_kernel.h):
 * 8-entry product tables for bit fields [0:3) and [3:6), 4-entry for
 * [6:8) — derived from the ISA-L lo/hi-nibble tables by GF linearity
 * over disjoint bits. */
static void pack_mixed_radix(const uint8_t *t, uint8_t *q) {
	for (int v = 0; v < 8; ++v) {
		q[v] = t[v];                                   /* c*v      */
		q[8 + v] = t[(8 * v) & 15] ^ t[16 + (v >> 1)]; /* c*(v<<3) */
	}
	for (int v = 0; v < 4; ++v)
		q[16 + v] = t[16 + (v << 2)];                  /* c*(v<<6) */
	memset(q + 20, 0, 12);
}

/* ------------------------------------------------------------------ */
/* CRC32 kernel                                                       */
/* ------------------------------------------------------------------ */

/* Device-constant block uploaded once per engine:
 *  [0..16*256)  u32: slicing tables T0..T15 (reflected, poly 0xEDB88320;
 *               the generic kernel uses T0..T3, the fast path T0..T7 by
 *               default or T0..T15 under LIZEC_CRC_SLICE=16)
 *  [then]       u32[26][32]: advance matrices M_i = "append 2^i zero
 *               BYTES", i = 0..25: zero runs shorter than 2^26 bytes,
 *               which bounds block_len below 2^27 (lizec_crc32_batch)    */
constexpr int kCrcTabWords = 16 * 256;  /* slicing-by-16 tables T0..T15 */
constexpr int kCrcMatCount = 26;
constexpr int kCrcConstWords = kCrcTabWords + kCrcMatCount * 32;

/* One wave per block: lane l owns segment [l*seg, l*seg+seg) of the block
 * (seg = block_len/64, multiple of 16 enforced by the host).  Lane 0 seeds;
 * the shfl tree folds 64 segment CRCs into the block CRC.  AL16=false
 * reads the buffer with dword loads, for bases that are only 4-byte
 * aligned (crc_ld16 in crc_fold.h). */
template <bool AL16 = true>
__global__ __launch_bounds__(kThreads) void crc32_blocks_kernel(
    const uint8_t *__restrict__ buf, uint32_t block_len, uint64_t nblocks,
    uint32_t seed, const uint32_t *__restrict__ crc_const,
    uint32_t *__restrict__ out) {
	__shared__ __attribute__((aligned(16))) uint32_t stabs[kCrcConstWords];
	for (int i = threadIdx.x; i < kCrcConstWords; i += kThreads)
		stabs[i] = crc_const[i];
	__syncthreads();
	const uint32_t *T0 = stabs;
	const uint32_t *T1 = stabs + 256;
	const uint32_t *T2 = stabs + 512;
	const uint32_t *T3 = stabs + 768;
	const uint32_t *mats = stabs + kCrcTabWords;

	const int wave = threadIdx.x >> 6;
	const int lane = threadIdx.x & 63;
	const uint32_t seg = block_len >> 6;   /* bytes per lane */

	for (uint64_t blk = (uint64_t)blockIdx.x * 4 + wave; blk < nblocks;
	     blk += (uint64_t)gridDim.x * 4) {
		const uint8_t *p = buf + blk * block_len + (uint32_t)lane * seg;
		uint32_t crc = (lane == 0 ? seed : 0u) ^ 0xFFFFFFFFu;
		for (uint32_t i = 0; i < seg; i += 16) {
			uint4 w = crc_ld16<AL16>(p + i);
#define LIZEC_CRC_WORD(x)                                              \
	do {                                                               \
		uint32_t u = crc ^ (x);                                        \
		crc = T3[u & 0xff] ^ T2[(u >> 8) & 0xff] ^                     \
		      T1[(u >> 16) & 0xff] ^ T0[u >> 24];                      \
	} while (0)
			LIZEC_CRC_WORD(w.x);
			LIZEC_CRC_WORD(w.y);
			LIZEC_CRC_WORD(w.z);
			LIZEC_CRC_WORD(w.w);
#undef LIZEC_CRC_WORD
		}
		crc ^= 0xFFFFFFFFu;

		/* fold: combine(cl, cr, len_r) = advance(cl, len_r) ^ cr */
		uint32_t len = seg;
#pragma unroll
		for (int s = 0; s < 6; ++s) {
			uint32_t ocrc = __shfl_down(crc, 1 << s, 64);
			uint32_t olen = __shfl_down(len, 1 << s, 64);
			crc = crc_advance(crc, olen, mats) ^ ocrc;
			len += olen;
		}
		if (lane == 0) out[blk] = crc;
	}
}

/* Fast path (block_len % 16384 == 0, e.g. the standard 64 KiB block):
 * one wave per block, C independent CRC chains per lane.  The block is cut
 * into C equal spans; lane l owns segment l of every span, so each lane
 * advances C serial CRC recurrences at once (ILP) and bursts BV*16
 * contiguous bytes per chain per iteration so every fetched line is
 * consumed while resident (the naive strided walk over-fetched HBM 2.2x
 * per the PMC counters).  Slicing-by-8 tables halve the dependent LDS
 * steps; per-lane CRCs fold in a shfl tree using the GF(2) "advance by N
 * zero bytes" matrices of mycrc32_combine (crc.cc:153-224), then lane 0
 * splices the C span CRCs. */
/* Per-wave CRC of one block: C chains x 64 lane segments, BV*16-byte
 * bursts, slicing-by-8; returns the block CRC on every lane (lane 0's
 * value is authoritative). */
template <int C, int BV, int SL = 16>
__device__ uint32_t crc_block_wave(const uint8_t *__restrict__ block,
                                   uint32_t block_len, uint32_t seed,
                                   const uint32_t *T, const uint32_t *mats,
                                   int lane) {
	const uint32_t span = block_len / C;
	const uint32_t seg = span >> 6;
	const uint8_t *base = block + (uint32_t)lane * seg;
	uint32_t crc[C];
#pragma unroll
	for (int c = 0; c < C; ++c)
		crc[c] = ((c == 0 && lane == 0) ? seed : 0u) ^ 0xFFFFFFFFu;
	for (uint32_t i = 0; i < seg; i += 16 * BV) {
		uint4 w[C][BV];
#pragma unroll
		for (int c = 0; c < C; ++c)
#pragma unroll
			for (int q = 0; q < BV; ++q)
				w[c][q] = *(const uint4 *)(base + c * span + i + q * 16);
/* one 16-byte step: 16 independent lookups per chain (slicing-by-16 —
 * the serial dependency is one LDS round trip per 16 bytes) */
#define LIZEC_CRC16(crc, v)                                              \
	do {                                                                 \
		uint32_t u0 = (crc) ^ (v).x, u1 = (v).y, u2 = (v).z, u3 = (v).w; \
		(crc) = T[15 * 256 + (u0 & 0xff)] ^                              \
		        T[14 * 256 + ((u0 >> 8) & 0xff)] ^                       \
		        T[13 * 256 + ((u0 >> 16) & 0xff)] ^                      \
		        T[12 * 256 + (u0 >> 24)] ^                               \
		        T[11 * 256 + (u1 & 0xff)] ^                              \
		        T[10 * 256 + ((u1 >> 8) & 0xff)] ^                       \
		        T[9 * 256 + ((u1 >> 16) & 0xff)] ^                       \
		        T[8 * 256 + (u1 >> 24)] ^                                \
		        T[7 * 256 + (u2 & 0xff)] ^                               \
		        T[6 * 256 + ((u2 >> 8) & 0xff)] ^                        \
		        T[5 * 256 + ((u2 >> 16) & 0xff)] ^                       \
		        T[4 * 256 + (u2 >> 24)] ^                                \
		        T[3 * 256 + (u3 & 0xff)] ^                               \
		        T[2 * 256 + ((u3 >> 8) & 0xff)] ^                        \
		        T[1 * 256 + ((u3 >> 16) & 0xff)] ^ T[u3 >> 24];          \
	} while (0)
#define LIZEC_CRC8(crc, lo, hi)                                          \
	do {                                                                 \
		uint32_t u0 = (crc) ^ (lo), u1 = (hi);                           \
		(crc) = T[7 * 256 + (u0 & 0xff)] ^                               \
		        T[6 * 256 + ((u0 >> 8) & 0xff)] ^                        \
		        T[5 * 256 + ((u0 >> 16) & 0xff)] ^                       \
		        T[4 * 256 + (u0 >> 24)] ^                                \
		        T[3 * 256 + (u1 & 0xff)] ^                               \
		        T[2 * 256 + ((u1 >> 8) & 0xff)] ^                        \
		        T[1 * 256 + ((u1 >> 16) & 0xff)] ^ T[u1 >> 24];          \
	} while (0)
#pragma unroll
		for (int q = 0; q < BV; ++q)
#pragma unroll
			for (int c = 0; c < C; ++c) {
				if (SL == 16) {
					LIZEC_CRC16(crc[c], w[c][q]);
				} else {
					LIZEC_CRC8(crc[c], w[c][q].x, w[c][q].y);
					LIZEC_CRC8(crc[c], w[c][q].z, w[c][q].w);
				}
			}
#undef LIZEC_CRC16
#undef LIZEC_CRC8
	}
#pragma unroll
	for (int c = 0; c < C; ++c) crc[c] ^= 0xFFFFFFFFu;

	uint32_t len = seg;
#pragma unroll
	for (int s = 0; s < 6; ++s) {
		uint32_t olen = __shfl_down(len, 1 << s, 64);
#pragma unroll
		for (int c = 0; c < C; ++c) {
			uint32_t o = __shfl_down(crc[c], 1 << s, 64);
			crc[c] = crc_advance(crc[c], olen, mats) ^ o;
		}
		len += olen;
	}
	uint32_t acc = crc[0];
#pragma unroll
	for (int c = 1; c < C; ++c)
		acc = crc_advance(acc, span, mats) ^ crc[c];
	return acc;
}

template <int C, int BV, int SL = 16>
__global__ __launch_bounds__(kThreads) void crc32_blocks_kernel_multi(
    const uint8_t *__restrict__ buf, uint32_t block_len, uint64_t nblocks,
    uint32_t seed, const uint32_t *__restrict__ crc_const,
    uint32_t *__restrict__ out) {
	__shared__ __attribute__((aligned(16))) uint32_t stabs[kCrcConstWords];
	for (int i = threadIdx.x; i < kCrcConstWords; i += kThreads)
		stabs[i] = crc_const[i];
	__syncthreads();
	const uint32_t *T = stabs;
	const uint32_t *mats = stabs + kCrcTabWords;
	const int wave = threadIdx.x >> 6;
	const int lane = threadIdx.x & 63;
	for (uint64_t blk = (uint64_t)blockIdx.x * 4 + wave; blk < nblocks;
	     blk += (uint64_t)gridDim.x * 4) {
		uint32_t crc = crc_block_wave<C, BV, SL>(buf + blk * block_len,
		                                         block_len, seed, T, mats,
		                                         lane);
		if (lane == 0) out[blk] = crc;
	}
}


/* LDS-free folding CRC kernel (crc_fold.h): the hot loop is pure VALU;
 * LDS holds only the epilogue byte table T0 and the combine matrices. */
constexpr int kCrcFoldLdsWords = 256 + kCrcMatCount * 32;

template <int C, int NACC, bool AL16 = true, bool NT = false,
          bool PF = false, int BVO = 0>
__global__ __launch_bounds__(kThreads) void crc32_blocks_kernel_fold(
    const uint8_t *__restrict__ buf, uint32_t block_len, uint64_t nblocks,
    uint32_t seed, const uint32_t *__restrict__ crc_const,
    uint32_t *__restrict__ out) {
	__shared__ __attribute__((aligned(16))) uint32_t stabs[kCrcFoldLdsWords];
	for (int i = threadIdx.x; i < 256; i += kThreads)
		stabs[i] = crc_const[i];
	for (int i = threadIdx.x; i < kCrcMatCount * 32; i += kThreads)
		stabs[256 + i] = crc_const[kCrcTabWords + i];
	__syncthreads();
	const int wave = threadIdx.x >> 6;
	const int lane = threadIdx.x & 63;
	for (uint64_t blk = (uint64_t)blockIdx.x * 4 + wave; blk < nblocks;
	     blk += (uint64_t)gridDim.x * 4) {
		uint32_t crc = crc_block_wave_fold<C, NACC, AL16, NT, PF, BVO>(
		    buf + blk * block_len, block_len, seed, stabs, stabs + 256, lane);
		if (lane == 0) out[blk] = crc;
	}
}

/* Batched chunk scrub / image-CRC fill.
 *
 * WRITE=false: hdd_int_test semantics (hddspacemgr.cc:2148-2212): for
 * every 64 KiB block of every chunk-part image, compare mycrc32(0, block,
 * MFSBLOCKSIZE) against the stored CRC array entry (big-endian u32 at
 * crc_off + crc_stride*b, cf. get32bit at hddspacemgr.cc:2183 and
 * chunk.cc:183-188).  status[c] collects the FIRST damaged block index
 * via atomicMin (host pre-fills INT32_MAX = clean).
 *
 * WRITE=true: image assembly for the replication pipeline
 * (chunk_replicator.cc:189 + chunk.cc:126-188): compute the same CRCs and
 * STORE them big-endian into the image's CRC array (status unused). */
template <bool WRITE>
__global__ __launch_bounds__(kThreads) void scrub_chunks_kernel(
    const uint64_t *__restrict__ chunk_dptrs,
    const uint32_t *__restrict__ data_offs,
    const uint32_t *__restrict__ crc_offs,
    const uint32_t *__restrict__ block_counts, uint32_t nchunks,
    uint32_t max_blocks, uint32_t block_stride, uint32_t crc_stride,
    const uint32_t *__restrict__ crc_const, int32_t *__restrict__ status) {
	__shared__ __attribute__((aligned(16))) uint32_t stabs[kCrcFoldLdsWords];
	for (int i = threadIdx.x; i < 256; i += kThreads)
		stabs[i] = crc_const[i];
	for (int i = threadIdx.x; i < kCrcMatCount * 32; i += kThreads)
		stabs[256 + i] = crc_const[kCrcTabWords + i];
	__syncthreads();
	const uint32_t *T0 = stabs;
	const uint32_t *mats = stabs + 256;
	const int wave = threadIdx.x >> 6;
	const int lane = threadIdx.x & 63;
	const uint64_t total = (uint64_t)nchunks * max_blocks;
	for (uint64_t flat = (uint64_t)blockIdx.x * 4 + wave; flat < total;
	     flat += (uint64_t)gridDim.x * 4) {
		uint32_t c = (uint32_t)(flat / max_blocks);
		uint32_t b = (uint32_t)(flat - (uint64_t)c * max_blocks);
		if (b >= block_counts[c]) continue;
		const uint8_t *img = (const uint8_t *)chunk_dptrs[c];
		const uint8_t *blockp = img + data_offs[c] + b * block_stride;
		/* INTERLEAVED-format blocks sit at 4 mod 16 — use the dword-load
		 * instantiation there (uint4 loads would be misaligned UB) */
		uint32_t crc =
		    (((uintptr_t)blockp & 15) == 0)
		        ? crc_block_wave_fold<1, 1, true>(blockp, 65536u, 0u, T0,
		                                          mats, lane)
		        : crc_block_wave_fold<1, 1, false>(blockp, 65536u, 0u, T0,
		                                           mats, lane);
		if (lane == 0) {
			uint8_t *p = (uint8_t *)img + crc_offs[c] + crc_stride * b;
			if (WRITE) {
				p[0] = (uint8_t)(crc >> 24);
				p[1] = (uint8_t)(crc >> 16);
				p[2] = (uint8_t)(crc >> 8);
				p[3] = (uint8_t)crc;
			} else {
				uint32_t stored = ((uint32_t)p[0] << 24) |
				                  ((uint32_t)p[1] << 16) |
				                  ((uint32_t)p[2] << 8) | p[3];
				if (stored != crc) atomicMin(&status[c], (int32_t)b);
			}
		}
	}
}

/* ------------------------------------------------------------------ */
/* Engine + plans                                                     */
/* ------------------------------------------------------------------ */

/* Per-stream call scratch.  The batch entry points upload tables/pointer
 * arrays into device scratch; keying the scratch by stream makes
 * concurrent calls on different streams of one engine race-free (the
 * chunkserver's bgjobs threading model is exactly multi-threaded,
 * network_main_thread.cc:230-234).  Within one stream, device scratch
 * reuse is stream-ordered; the pinned host staging buffer is guarded by
 * an event recorded after the H2D copies are enqueued. */
struct lizec_stream_ctx {
	uint8_t *d_gftbls = nullptr;    /* 16*32*32 (packed quarter-LUT) */
	uint64_t *d_ptrs = nullptr;     /* grows */
	size_t ptrs_cap = 0;            /* in elements */
	uint8_t *h_staging = nullptr;   /* pinned: tables + pointer arrays */
	size_t h_cap = 0;               /* staging bytes */
	hipEvent_t uploaded = nullptr;  /* staging consumed up to here */
	bool ev_recorded = false;
	/* multi-table batches only (lizec_ec_encode_batch_multi): per-stripe
	 * table index and the packed tables, with a pinned staging buffer of
	 * their own; guarded by the same `uploaded` event.  Never allocated
	 * for callers of the single-table entry points. */
	uint8_t *d_mtbls = nullptr;     /* ntables packed tables, grows */
	size_t mtbls_cap = 0;           /* bytes */
	uint32_t *d_mindex = nullptr;   /* tbl_index, grows */
	size_t mindex_cap = 0;          /* in elements */
	uint8_t *h_mstaging = nullptr;  /* pinned: packed tables + index */
	size_t h_mcap = 0;              /* bytes */
	/* ragged batches only (lizec_ec_encode_batch_ragged): one device buffer
	 * holding packed tables, table index, block map and the two block-count
	 * arrays, and its pinned mirror; guarded by the same `uploaded` event.
	 * Never allocated for callers of the other entry points. */
	uint8_t *d_ragged = nullptr;    /* grows */
	uint8_t *h_ragged = nullptr;    /* pinned, same size */
	size_t ragged_cap = 0;          /* bytes */
};

struct lizec_engine {
	int device;
	hipStream_t stream;        /* default stream for calls passing NULL */
	uint32_t *d_crc_const;     /* kCrcConstWords */
	std::mutex mu;             /* guards ctxs */
	std::unordered_map<void *, lizec_stream_ctx> ctxs;
	/* CRC fold shape, autotuned on the first large batch: -1 undecided,
	 * 0 = no-prefetch (5 waves/SIMD, robust), 1 = burst-prefetch
	 * (2 waves; +6-7% on most boxes, -20% on some — profiles/ROUND2.md) */
	std::atomic<int> crc_shape{-1};
};

static void ctx_free(lizec_stream_ctx &c) {
	(void)hipFree(c.d_gftbls);
	(void)hipFree(c.d_ptrs);
	(void)hipHostFree(c.h_staging);
	(void)hipFree(c.d_mtbls);
	(void)hipFree(c.d_mindex);
	(void)hipHostFree(c.h_mstaging);
	(void)hipFree(c.d_ragged);
	(void)hipHostFree(c.h_ragged);
	if (c.uploaded) (void)hipEventDestroy(c.uploaded);
	c = lizec_stream_ctx();
}

/* Get (or create) the scratch for `s`, sized for `ptrs` pointer slots and
 * `staging` staging bytes; waits out any still-pending staging use.
 * Thread contract: concurrent calls must use distinct streams (each
 * stream's scratch is touched by one call at a time — the map lookup is
 * the only globally locked step, so streams never stall each other). */
static int ctx_acquire(lizec_engine *e, hipStream_t s, size_t ptrs,
                       size_t staging, lizec_stream_ctx **out) {
	lizec_stream_ctx *cp;
	{
		std::lock_guard<std::mutex> lk(e->mu);
		cp = &e->ctxs[(void *)s];   /* element refs survive rehash */
	}
	lizec_stream_ctx &c = *cp;
	if (!c.uploaded) {
		if (hipEventCreateWithFlags(&c.uploaded, hipEventDisableTiming) !=
		    hipSuccess)
			return LIZEC_EHIP;
	}
	if (c.ev_recorded) {
		/* previous call on this stream may still be reading h_staging (and
		 * a grow below would free device scratch it reads) — wait it out */
		LIZEC_CHECK(hipEventSynchronize(c.uploaded));
		c.ev_recorded = false;
	}
	if (!c.d_gftbls)
		LIZEC_CHECK(hipMalloc(&c.d_gftbls, (size_t)kECTblBytes * 32 * 32));
	if (c.ptrs_cap < ptrs) {
		size_t cap = c.ptrs_cap ? c.ptrs_cap : (1 << 16);
		while (cap < ptrs) cap *= 2;
		(void)hipFree(c.d_ptrs);
		c.d_ptrs = nullptr;
		c.ptrs_cap = 0;
		LIZEC_CHECK(hipMalloc(&c.d_ptrs, cap * sizeof(uint64_t)));
		c.ptrs_cap = cap;
	}
	size_t want = staging + (size_t)kECTblBytes * 32 * 32;
	if (c.h_cap < want) {
		size_t cap = c.h_cap ? c.h_cap : (1 << 20);
		while (cap < want) cap *= 2;
		(void)hipHostFree(c.h_staging);
		c.h_staging = nullptr;
		c.h_cap = 0;
		LIZEC_CHECK(hipHostMalloc(&c.h_staging, cap));
		c.h_cap = cap;
	}
	*out = &c;
	return LIZEC_OK;
}

/* ctx_acquire plus the multi-table scratch: `tbl_bytes` of packed tables
 * and `stripes` index entries on the device, and pinned staging for both.
 * ctx_acquire has already waited out the previous call's uploads, so the
 * buffers are free to grow (hipFree itself waits for running kernels). */
static int ctx_acquire_multi(lizec_engine *e, hipStream_t s, size_t ptrs,
                             size_t staging, size_t tbl_bytes, size_t stripes,
                             lizec_stream_ctx **out) {
	int r = ctx_acquire(e, s, ptrs, staging, out);
	if (r != LIZEC_OK) return r;
	lizec_stream_ctx &c = **out;
	if (c.mtbls_cap < tbl_bytes) {
		size_t cap = c.mtbls_cap ? c.mtbls_cap : (1 << 16);
		while (cap < tbl_bytes) cap *= 2;
		(void)hipFree(c.d_mtbls);
		c.d_mtbls = nullptr;
		c.mtbls_cap = 0;
		LIZEC_CHECK(hipMalloc(&c.d_mtbls, cap));
		c.mtbls_cap = cap;
	}
	if (c.mindex_cap < stripes) {
		size_t cap = c.mindex_cap ? c.mindex_cap : (1 << 14);
		while (cap < stripes) cap *= 2;
		(void)hipFree(c.d_mindex);
		c.d_mindex = nullptr;
		c.mindex_cap = 0;
		LIZEC_CHECK(hipMalloc(&c.d_mindex, cap * sizeof(uint32_t)));
		c.mindex_cap = cap;
	}
	size_t want = tbl_bytes + stripes * sizeof(uint32_t);
	if (c.h_mcap < want) {
		size_t cap = c.h_mcap ? c.h_mcap : (1 << 17);
		while (cap < want) cap *= 2;
		(void)hipHostFree(c.h_mstaging);
		c.h_mstaging = nullptr;
		c.h_mcap = 0;
		LIZEC_CHECK(hipHostMalloc(&c.h_mstaging, cap));
		c.h_mcap = cap;
	}
	return LIZEC_OK;
}

/* ctx_acquire plus the ragged scratch: `bytes` on the device and as many
 * pinned.  As in ctx_acquire_multi the previous call's uploads are over. */
static int ctx_acquire_ragged(lizec_engine *e, hipStream_t s, size_t ptrs,
                              size_t staging, size_t bytes,
                              lizec_stream_ctx **out) {
	int r = ctx_acquire(e, s, ptrs, staging, out);
	if (r != LIZEC_OK) return r;
	lizec_stream_ctx &c = **out;
	if (c.ragged_cap < bytes) {
		size_t cap = c.ragged_cap ? c.ragged_cap : (1 << 17);
		while (cap < bytes) cap *= 2;
		(void)hipFree(c.d_ragged);
		(void)hipHostFree(c.h_ragged);
		c.d_ragged = c.h_ragged = nullptr;
		c.ragged_cap = 0;
		LIZEC_CHECK(hipMalloc(&c.d_ragged, cap));
		LIZEC_CHECK(hipHostMalloc(&c.h_ragged, cap));
		c.ragged_cap = cap;
	}
	return LIZEC_OK;
}

/* A plan = a prepared batch: device-resident tables + pointer arrays.
 * Mirrors the reference's cached-matrix + read-plan structure
 * (reed_solomon.h:194-198, read_plan.h): build once per (erasure pattern,
 * batch), run many times with zero host->device traffic. */
struct lizec_plan {
	lizec_engine *e;
	uint64_t part_len;
	int srcs, dests, num_stripes;
	uint8_t *d_tbls;
	uint64_t *d_src;
	uint64_t *d_dst;
	uint32_t *d_index;   /* multi-table plans only: per-stripe table index */
};

extern "C" int lizec_gpu_count(void) {
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

/* Build the CRC constant block on the host (product-side tables; bit-exact
 * semantics enforced by tests vs the oracle). */
static void build_crc_const(uint32_t *w) {
	for (uint32_t i = 0; i < 256; ++i) {
		uint32_t c = i;
		for (int b = 0; b < 8; ++b)
			c = (c & 1) ? (0xEDB88320u ^ (c >> 1)) : (c >> 1);
		w[i] = c;
	}
	for (uint32_t i = 0; i < 256; ++i)
		for (int t = 1; t < 16; ++t) {
			uint32_t c = w[(t - 1) * 256 + i];
			w[t * 256 + i] = w[c & 0xff] ^ (c >> 8);
		}
	/* advance matrices: M_0 = 1 zero byte; M_{i+1} = M_i^2 */
	uint32_t *mats = w + kCrcTabWords;
	uint32_t odd[32], even[32];
	odd[0] = 0xEDB88320u;                 /* 1 zero BIT */
	for (int i = 1; i < 32; ++i) odd[i] = 1u << (i - 1);
	auto times = [](const uint32_t *m, uint32_t v) {
		uint32_t s = 0;
		for (int i = 0; v; v >>= 1, ++i)
			if (v & 1) s ^= m[i];
		return s;
	};
	auto square = [&](uint32_t *sq, const uint32_t *m) {
		for (int i = 0; i < 32; ++i) sq[i] = times(m, m[i]);
	};
	square(even, odd);    /* 2 bits */
	square(odd, even);    /* 4 bits */
	square(even, odd);    /* 8 bits = 1 byte -> M_0 */
	memcpy(mats, even, 32 * 4);
	for (int i = 1; i < kCrcMatCount; ++i) {
		square(odd, (uint32_t *)(mats + (i - 1) * 32));
		memcpy(mats + i * 32, odd, 32 * 4);
	}
}

extern "C" int lizec_engine_create(lizec_engine **out, int device_id) {
	*out = nullptr;
	int n = lizec_gpu_count();
	if (n <= 0 || device_id >= n) return LIZEC_ENOGPU;
	LIZEC_CHECK(hipSetDevice(device_id));
	lizec_engine *e = new lizec_engine();
	e->device = device_id;
	if (hipStreamCreate(&e->stream) != hipSuccess ||
	    hipMalloc(&e->d_crc_const, kCrcConstWords * 4) != hipSuccess) {
		lizec_engine_destroy(e);   /* frees whatever was allocated */
		return LIZEC_ENOMEM;
	}
	uint32_t *host_const = (uint32_t *)malloc(kCrcConstWords * 4);
	build_crc_const(host_const);
	hipError_t err = hipMemcpy(e->d_crc_const, host_const, kCrcConstWords * 4,
	                           hipMemcpyHostToDevice);
	free(host_const);
	if (err != hipSuccess) {
		lizec_engine_destroy(e);
		return LIZEC_EHIP;
	}
	*out = e;
	return LIZEC_OK;
}

extern "C" void lizec_engine_destroy(lizec_engine *e) {
	if (!e) return;
	for (auto &kv : e->ctxs) ctx_free(kv.second);
	(void)hipFree(e->d_crc_const);
	(void)hipStreamDestroy(e->stream);
	delete e;
}

extern "C" int lizec_engine_sync(lizec_engine *e) {
	LIZEC_CHECK(hipSetDevice(e->device));
	LIZEC_CHECK(hipStreamSynchronize(e->stream));
	return LIZEC_OK;
}

static int check_batch_args(uint64_t part_len, int srcs, int dests,
                            int num_stripes) {
	if (srcs < 1 || srcs > 32 || dests < 1 || dests > 32 || num_stripes < 1)
		return LIZEC_EINVAL;
	if (part_len == 0 || (part_len & 15) || part_len > (uint64_t)1 << 31)
		return LIZEC_EINVAL;
	return LIZEC_OK;
}

/* The kernels read and write every part with 16-byte vector accesses at
 * 16-byte offsets, so every part address must be 16-byte aligned (0, the
 * multi-table "skip this output", passes).  Host only, before anything is
 * allocated or enqueued. */
static int check_part_addrs(const uint64_t *src_dptrs, size_t nsrc,
                            const uint64_t *dst_dptrs, size_t ndst) {
	uint64_t bits = 0;
	for (size_t i = 0; i < nsrc; ++i) bits |= src_dptrs[i];
	for (size_t i = 0; i < ndst; ++i) bits |= dst_dptrs[i];
	return (bits & 15) ? LIZEC_EINVAL : LIZEC_OK;
}

template <int D>
static void launch_ec(uint32_t part_len, int srcs, int dest_base,
                      const uint8_t *d_tbls, const uint64_t *d_src,
                      const uint64_t *d_dst, int dests_total,
                      uint32_t tiles_per_part_unused, uint32_t nstripes,
                      hipStream_t s) {
	constexpr int CH = ec_chunks_for(D);
	uint32_t tile_bytes = kChunkBytes * CH;
	uint32_t tiles_per_part = (part_len + tile_bytes - 1) / tile_bytes;
	uint32_t total_tiles = tiles_per_part * nstripes;
	uint32_t grid = total_tiles < 1048576u ? total_tiles : 1048576u;   /* exact grid (1 tile/block) measured +0.7% */
	size_t lds = (size_t)D * srcs * kECTblBytes;
	(void)tiles_per_part_unused;
	hipLaunchKernelGGL(HIP_KERNEL_NAME(ec_encode_kernel<D, CH, kECSwz, kECNtStore, kECNtLoad, false, false, true>),
	                   dim3(grid), dim3(kThreads), lds, s,
	                   part_len, srcs, dest_base, d_tbls, d_src, d_dst,
	                   dests_total, tiles_per_part, total_tiles);
}

static int run_batch(uint64_t part_len, int srcs, int dests,
                     const uint8_t *d_tbls, const uint64_t *d_src,
                     const uint64_t *d_dst, uint32_t num_stripes,
                     hipStream_t s) {
	/* One pass computes up to kMaxDestsPerPass destinations; wider m splits
	 * into passes (each pass re-reads the sources, so fewer passes wins on
	 * this HBM-bound kernel — D<=8 measured best, profiles/). */
	for (int base = 0; base < dests;) {
		int d = dests - base;
		if (d > 8) d = 8;
		switch (d) {
		case 1: launch_ec<1>((uint32_t)part_len, srcs, base, d_tbls, d_src,
		                     d_dst, dests, 0, num_stripes, s);
			break;
		case 2: launch_ec<2>((uint32_t)part_len, srcs, base, d_tbls, d_src,
		                     d_dst, dests, 0, num_stripes, s);
			break;
		case 3: launch_ec<3>((uint32_t)part_len, srcs, base, d_tbls, d_src,
		                     d_dst, dests, 0, num_stripes, s);
			break;
		case 4: launch_ec<4>((uint32_t)part_len, srcs, base, d_tbls, d_src,
		                     d_dst, dests, 0, num_stripes, s);
			break;
		case 5: launch_ec<5>((uint32_t)part_len, srcs, base, d_tbls, d_src,
		                     d_dst, dests, 0, num_stripes, s);
			break;
		case 6: launch_ec<6>((uint32_t)part_len, srcs, base, d_tbls, d_src,
		                     d_dst, dests, 0, num_stripes, s);
			break;
		case 7: launch_ec<7>((uint32_t)part_len, srcs, base, d_tbls, d_src,
		                     d_dst, dests, 0, num_stripes, s);
			break;
		default: launch_ec<8>((uint32_t)part_len, srcs, base, d_tbls, d_src,
		                      d_dst, dests, 0, num_stripes, s);
			break;
		}
		base += d;
	}
	LIZEC_CHECK(hipGetLastError());
	return LIZEC_OK;
}

/* Upload one table and the two pointer arrays of a single-table batch
 * through the stream's scratch; on success *d_src / *d_dst are the device
 * pointer arrays and c->d_gftbls the packed table. */
static int upload_single_table(lizec_engine *e, hipStream_t s, int srcs,
                               int dests, const uint8_t *gftbls,
                               const uint64_t *src_dptrs, size_t nsrc,
                               const uint64_t *dst_dptrs, size_t ndst,
                               lizec_stream_ctx **ctx, uint64_t **d_src,
                               uint64_t **d_dst) {
	lizec_stream_ctx *c;
	int r = ctx_acquire(e, s, nsrc + ndst, (nsrc + ndst) * 8, &c);
	if (r != LIZEC_OK) return r;
	*ctx = c;
	*d_src = c->d_ptrs;
	*d_dst = c->d_ptrs + nsrc;
	/* stage tables + pointer arrays through this stream's pinned buffer
	 * (ctx_acquire waited until any previous copies from it finished) */
	uint8_t *tstage = c->h_staging;
	uint64_t *pstage = (uint64_t *)(c->h_staging + (size_t)kECTblBytes * 32 * 32);
	for (int i = 0; i < srcs * dests; ++i)
		pack_mixed_radix(gftbls + (size_t)i * 32, tstage + (size_t)i * kECTblBytes);
	memcpy(pstage, src_dptrs, nsrc * 8);
	memcpy(pstage + nsrc, dst_dptrs, ndst * 8);
	LIZEC_CHECK(hipMemcpyAsync(c->d_gftbls, tstage, (size_t)kECTblBytes * srcs * dests,
	                           hipMemcpyHostToDevice, s));
	LIZEC_CHECK(hipMemcpyAsync(*d_src, pstage, (nsrc + ndst) * 8,
	                           hipMemcpyHostToDevice, s));
	LIZEC_CHECK(hipEventRecord(c->uploaded, s));
	c->ev_recorded = true;
	return LIZEC_OK;
}

extern "C" int lizec_ec_encode_batch(lizec_engine *e, uint64_t part_len,
                                     int srcs, int dests,
                                     const uint8_t *gftbls,
                                     const uint64_t *src_dptrs,
                                     const uint64_t *dst_dptrs,
                                     int num_stripes, void *stream) {
	if (!e) return LIZEC_EINVAL;
	int r = check_batch_args(part_len, srcs, dests, num_stripes);
	if (r != LIZEC_OK) return r;
	size_t nsrc = (size_t)num_stripes * srcs;
	size_t ndst = (size_t)num_stripes * dests;
	r = check_part_addrs(src_dptrs, nsrc, dst_dptrs, ndst);
	if (r != LIZEC_OK) return r;
	hipStream_t s = stream ? (hipStream_t)stream : e->stream;
	LIZEC_CHECK(hipSetDevice(e->device));

	lizec_stream_ctx *c;
	uint64_t *d_src, *d_dst;
	r = upload_single_table(e, s, srcs, dests, gftbls, src_dptrs, nsrc,
	                        dst_dptrs, ndst, &c, &d_src, &d_dst);
	if (r != LIZEC_OK) return r;
	return run_batch(part_len, srcs, dests, c->d_gftbls, d_src, d_dst,
	                 (uint32_t)num_stripes, s);
}

/* ------------------------------------------------------------------ */
/* Block-strided, 4-byte-aligned parts (ec_kernel_strided.h)          */
/* ------------------------------------------------------------------ */

/* One pass of the strided kernel: exactly one workgroup per tile. */
template <int D>
static void launch_ec_strided(uint32_t nblocks, int srcs, int dest_base,
                              const uint8_t *d_tbls, const uint64_t *d_src,
                              const uint64_t *d_dst, int dests_total,
                              uint32_t nstripes, uint32_t src_stride,
                              uint32_t dst_stride, bool sal, bool dal,
                              hipStream_t s) {
	constexpr int CH = ec_chunks_for(D);
	uint32_t tiles_per_part = nblocks * (kECBlockBytes / (kChunkBytes * CH));
	uint32_t total_tiles = tiles_per_part * nstripes;
	size_t lds = (size_t)D * srcs * kECTblBytes;
#define LIZEC_LAUNCH_STRIDED(SAL, DAL)                                      \
	hipLaunchKernelGGL(HIP_KERNEL_NAME(ec_encode_strided_kernel<D, CH, SAL, DAL>), \
	                   dim3(total_tiles), dim3(kThreads), lds, s,           \
	                   tiles_per_part, srcs, dest_base, d_tbls, d_src,      \
	                   d_dst, dests_total, src_stride, dst_stride)
	if (sal && dal) LIZEC_LAUNCH_STRIDED(true, true);
	else if (sal) LIZEC_LAUNCH_STRIDED(true, false);
	else if (dal) LIZEC_LAUNCH_STRIDED(false, true);
	else LIZEC_LAUNCH_STRIDED(false, false);
#undef LIZEC_LAUNCH_STRIDED
}

/* Largest batch of the strided kernel, counted in 8 KiB tiles (the smaller
 * of the two tile sizes): the grid is one workgroup per tile. */
static bool strided_tiles_fit(uint32_t nblocks, uint32_t num_stripes) {
	return (uint64_t)nblocks * (kECBlockBytes / (kChunkBytes * 2)) *
	           num_stripes <= 0x7FFFFFFFull;
}

/* run_batch for strided parts: the same split into passes of at most 8
 * destinations.  sal / dal: that side is 16-byte aligned throughout. */
static int run_batch_strided(uint32_t nblocks, int srcs, int dests,
                             const uint8_t *d_tbls, const uint64_t *d_src,
                             const uint64_t *d_dst, uint32_t num_stripes,
                             uint32_t src_stride, uint32_t dst_stride,
                             bool sal, bool dal, hipStream_t s) {
	if (!strided_tiles_fit(nblocks, num_stripes)) return LIZEC_EINVAL;
	for (int base = 0; base < dests;) {
		int d = dests - base;
		if (d > 8) d = 8;
#define LIZEC_LAUNCH_STRIDED_D(D)                                          \
	launch_ec_strided<D>(nblocks, srcs, base, d_tbls, d_src, d_dst, dests, \
	                     num_stripes, src_stride, dst_stride, sal, dal, s)
		switch (d) {
		case 1: LIZEC_LAUNCH_STRIDED_D(1); break;
		case 2: LIZEC_LAUNCH_STRIDED_D(2); break;
		case 3: LIZEC_LAUNCH_STRIDED_D(3); break;
		case 4: LIZEC_LAUNCH_STRIDED_D(4); break;
		case 5: LIZEC_LAUNCH_STRIDED_D(5); break;
		case 6: LIZEC_LAUNCH_STRIDED_D(6); break;
		case 7: LIZEC_LAUNCH_STRIDED_D(7); break;
		default: LIZEC_LAUNCH_STRIDED_D(8); break;
		}
#undef LIZEC_LAUNCH_STRIDED_D
		base += d;
	}
	LIZEC_CHECK(hipGetLastError());
	return LIZEC_OK;
}

extern "C" int lizec_ec_encode_batch_strided(
    lizec_engine *e, uint32_t nblocks, int srcs, int dests,
    const uint8_t *gftbls, const uint64_t *src_dptrs,
    const uint64_t *dst_dptrs, int num_stripes, uint32_t src_block_stride,
    uint32_t dst_block_stride, void *stream) {
	if (!e || !gftbls || !src_dptrs || !dst_dptrs) return LIZEC_EINVAL;
	if (srcs < 1 || srcs > 32 || dests < 1 || dests > 32 || num_stripes < 1)
		return LIZEC_EINVAL;
	if (nblocks == 0 || (uint64_t)nblocks * kECBlockBytes > (uint64_t)1 << 31)
		return LIZEC_EINVAL;
	if (src_block_stride < kECBlockBytes || dst_block_stride < kECBlockBytes)
		return LIZEC_EINVAL;
	if (!strided_tiles_fit(nblocks, (uint32_t)num_stripes))
		return LIZEC_EINVAL;
	size_t nsrc = (size_t)num_stripes * srcs;
	size_t ndst = (size_t)num_stripes * dests;
	/* every address nonzero; per side, the OR of addresses and stride
	 * decides between refusal (not 4-byte aligned), the dword-aligned
	 * kernel forms, and the 16-byte-aligned ones */
	uint64_t sbits = src_block_stride, dbits = dst_block_stride;
	for (size_t i = 0; i < nsrc; ++i) {
		if (!src_dptrs[i]) return LIZEC_EINVAL;
		sbits |= src_dptrs[i];
	}
	for (size_t i = 0; i < ndst; ++i) {
		if (!dst_dptrs[i]) return LIZEC_EINVAL;
		dbits |= dst_dptrs[i];
	}
	if ((sbits | dbits) & 3) return LIZEC_EINVAL;
	const bool sal = (sbits & 15) == 0, dal = (dbits & 15) == 0;
	hipStream_t s = stream ? (hipStream_t)stream : e->stream;
	LIZEC_CHECK(hipSetDevice(e->device));

	lizec_stream_ctx *c;
	uint64_t *d_src, *d_dst;
	int r = upload_single_table(e, s, srcs, dests, gftbls, src_dptrs, nsrc,
	                            dst_dptrs, ndst, &c, &d_src, &d_dst);
	if (r != LIZEC_OK) return r;
	/* contiguous, fully aligned parts are the uniform kernel's case */
	if (sal && dal && src_block_stride == kECBlockBytes &&
	    dst_block_stride == kECBlockBytes)
		return run_batch((uint64_t)nblocks * kECBlockBytes, srcs, dests,
		                 c->d_gftbls, d_src, d_dst, (uint32_t)num_stripes, s);
	return run_batch_strided(nblocks, srcs, dests, c->d_gftbls, d_src, d_dst,
	                         (uint32_t)num_stripes, src_block_stride,
	                         dst_block_stride, sal, dal, s);
}

/* ------------------------------------------------------------------ */
/* Ragged batches: a block count per part (ec_kernel_ragged.h)        */
/* ------------------------------------------------------------------ */

struct ragged_dev {
	const uint8_t *tbls;
	const uint32_t *index;
	const uint2 *map;
	const uint64_t *src, *dst;
	const uint32_t *src_nb, *dst_nb;
};

/* One pass of the ragged kernel: one workgroup per tile of every block row
 * in the map. */
template <int D>
static void launch_ec_ragged(uint32_t entries, int srcs, int dest_base,
                             const ragged_dev &r, int dests_total,
                             uint32_t src_stride, uint32_t dst_stride,
                             bool sal, bool dal, hipStream_t s) {
	constexpr int CH = ec_chunks_for(D);
	uint32_t total_tiles = entries * (kECBlockBytes / (kChunkBytes * CH));
	size_t lds = (size_t)D * srcs * kECTblBytes;
#define LIZEC_LAUNCH_RAGGED(SAL, DAL)                                       \
	hipLaunchKernelGGL(HIP_KERNEL_NAME(ec_encode_ragged_kernel<D, CH, SAL, DAL>), \
	                   dim3(total_tiles), dim3(kThreads), lds, s, srcs,     \
	                   dest_base, r.tbls, r.index, r.map, r.src, r.src_nb,  \
	                   r.dst, r.dst_nb, dests_total, src_stride, dst_stride)
	if (sal && dal) LIZEC_LAUNCH_RAGGED(true, true);
	else if (sal) LIZEC_LAUNCH_RAGGED(true, false);
	else if (dal) LIZEC_LAUNCH_RAGGED(false, true);
	else LIZEC_LAUNCH_RAGGED(false, false);
#undef LIZEC_LAUNCH_RAGGED
}

/* Every pass of a ragged batch: at most 8 destinations each, as
 * run_batch_strided.  Shared by lizec_ec_encode_batch_ragged and the ragged
 * streaming rebuild, which keeps the device arrays in its own slots. */
static void launch_ec_ragged_passes(uint32_t entries, int srcs, int dests,
                                    const ragged_dev &rd,
                                    uint32_t src_block_stride,
                                    uint32_t dst_block_stride, bool sal,
                                    bool dal, hipStream_t s) {
	for (int base = 0; base < dests;) {
		int d = dests - base;
		if (d > 8) d = 8;
#define LIZEC_LAUNCH_RAGGED_D(D)                                           \
	launch_ec_ragged<D>(entries, srcs, base, rd, dests, src_block_stride,  \
	                    dst_block_stride, sal, dal, s)
		switch (d) {
		case 1: LIZEC_LAUNCH_RAGGED_D(1); break;
		case 2: LIZEC_LAUNCH_RAGGED_D(2); break;
		case 3: LIZEC_LAUNCH_RAGGED_D(3); break;
		case 4: LIZEC_LAUNCH_RAGGED_D(4); break;
		case 5: LIZEC_LAUNCH_RAGGED_D(5); break;
		case 6: LIZEC_LAUNCH_RAGGED_D(6); break;
		case 7: LIZEC_LAUNCH_RAGGED_D(7); break;
		default: LIZEC_LAUNCH_RAGGED_D(8); break;
		}
#undef LIZEC_LAUNCH_RAGGED_D
		base += d;
	}
}

extern "C" int lizec_ec_encode_batch_ragged(
    lizec_engine *e, int srcs, int dests, const uint8_t *gftbls, int ntables,
    const uint32_t *tbl_index, const uint64_t *src_dptrs,
    const uint32_t *src_nblocks, const uint64_t *dst_dptrs,
    const uint32_t *dst_nblocks, int num_stripes, uint32_t src_block_stride,
    uint32_t dst_block_stride, void *stream) {
	if (!e || !gftbls || !src_dptrs || !src_nblocks || !dst_dptrs ||
	    !dst_nblocks)
		return LIZEC_EINVAL;
	if (srcs < 1 || srcs > 32 || dests < 1 || dests > 32 || num_stripes < 1)
		return LIZEC_EINVAL;
	if (ntables < 1 ||
	    (uint64_t)ntables * 32 * srcs * dests > (uint64_t)1 << 30)
		return LIZEC_EINVAL;
	if (src_block_stride < kECBlockBytes || dst_block_stride < kECBlockBytes)
		return LIZEC_EINVAL;
	if (tbl_index)
		for (int i = 0; i < num_stripes; ++i)
			if (tbl_index[i] >= (uint32_t)ntables) return LIZEC_EINVAL;
	size_t nsrc = (size_t)num_stripes * srcs;
	size_t ndst = (size_t)num_stripes * dests;
	/* per side, the OR of the stride and of the addresses that are used
	 * (count > 0) decides between refusal, the dword-aligned kernel forms
	 * and the 16-byte-aligned ones; an unused address may be anything */
	uint64_t sbits = src_block_stride, dbits = dst_block_stride;
	for (size_t i = 0; i < nsrc; ++i) {
		if (src_nblocks[i] > 32768u) return LIZEC_EINVAL;
		if (!src_nblocks[i]) continue;
		if (!src_dptrs[i]) return LIZEC_EINVAL;
		sbits |= src_dptrs[i];
	}
	for (size_t i = 0; i < ndst; ++i) {
		if (dst_nblocks[i] > 32768u) return LIZEC_EINVAL;
		if (!dst_nblocks[i]) continue;
		if (!dst_dptrs[i]) return LIZEC_EINVAL;
		dbits |= dst_dptrs[i];
	}
	if ((sbits | dbits) & 3) return LIZEC_EINVAL;
	const bool sal = (sbits & 15) == 0, dal = (dbits & 15) == 0;
	/* counts the block rows and refuses a batch of more than 2^31-1 tiles */
	int64_t entries =
	    lizec_ragged_block_map(dst_nblocks, dests, num_stripes, nullptr, 0);
	if (entries <= 0) return LIZEC_EINVAL;
	hipStream_t s = stream ? (hipStream_t)stream : e->stream;
	LIZEC_CHECK(hipSetDevice(e->device));

	/* scratch layout, every section 16-byte aligned */
	auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
	size_t ntbl = (size_t)ntables * srcs * dests;   /* 32-byte tables */
	size_t o_index = up16(ntbl * kECTblBytes);
	size_t o_map = o_index + up16((size_t)num_stripes * 4);
	size_t o_snb = o_map + up16((size_t)entries * 8);
	size_t o_dnb = o_snb + up16(nsrc * 4);
	size_t bytes = o_dnb + up16(ndst * 4);
	lizec_stream_ctx *c;
	int r = ctx_acquire_ragged(e, s, nsrc + ndst, (nsrc + ndst) * 8, bytes, &c);
	if (r != LIZEC_OK) return r;
	uint8_t *h = c->h_ragged;
	for (size_t i = 0; i < ntbl; ++i)
		pack_mixed_radix(gftbls + i * 32, h + i * kECTblBytes);
	if (tbl_index)
		memcpy(h + o_index, tbl_index, (size_t)num_stripes * 4);
	else
		memset(h + o_index, 0, (size_t)num_stripes * 4);
	if (lizec_ragged_block_map(dst_nblocks, dests, num_stripes,
	                           (uint32_t *)(h + o_map),
	                           (uint64_t)entries) != entries)
		return LIZEC_EINVAL;
	memcpy(h + o_snb, src_nblocks, nsrc * 4);
	memcpy(h + o_dnb, dst_nblocks, ndst * 4);
	uint64_t *pstage = (uint64_t *)(c->h_staging + (size_t)kECTblBytes * 32 * 32);
	memcpy(pstage, src_dptrs, nsrc * 8);
	memcpy(pstage + nsrc, dst_dptrs, ndst * 8);
	LIZEC_CHECK(hipMemcpyAsync(c->d_ragged, h, bytes, hipMemcpyHostToDevice, s));
	LIZEC_CHECK(hipMemcpyAsync(c->d_ptrs, pstage, (nsrc + ndst) * 8,
	                           hipMemcpyHostToDevice, s));
	LIZEC_CHECK(hipEventRecord(c->uploaded, s));
	c->ev_recorded = true;

	ragged_dev rd;
	rd.tbls = c->d_ragged;
	rd.index = (const uint32_t *)(c->d_ragged + o_index);
	rd.map = (const uint2 *)(c->d_ragged + o_map);
	rd.src_nb = (const uint32_t *)(c->d_ragged + o_snb);
	rd.dst_nb = (const uint32_t *)(c->d_ragged + o_dnb);
	rd.src = c->d_ptrs;
	rd.dst = c->d_ptrs + nsrc;
	launch_ec_ragged_passes((uint32_t)entries, srcs, dests, rd,
	                        src_block_stride, dst_block_stride, sal, dal, s);
	LIZEC_CHECK(hipGetLastError());
	return LIZEC_OK;
}

/* ------------------------------------------------------------------ */
/* Chunk views: parts cut from a chunk held in another slice type     */
/* (ec_kernel_view.h)                                                 */
/* ------------------------------------------------------------------ */

struct view_dev {
	const uint8_t *tbls;
	const uint32_t *index;
	const uint2 *map;
	const uint64_t *view, *dst;
	const uint32_t *chunk_nb, *col0, *dst_nb;
	uint32_t view_parts, row_cols;
};

/* One pass of the view kernel: the grid of launch_ec_ragged. */
template <int D>
static void launch_ec_view(uint32_t entries, int srcs, int dest_base,
                           const view_dev &v, int dests_total,
                           uint32_t src_stride, uint32_t dst_stride,
                           bool sal, bool dal, hipStream_t s) {
	constexpr int CH = ec_chunks_for(D);
	uint32_t total_tiles = entries * (kECBlockBytes / (kChunkBytes * CH));
	size_t lds = (size_t)D * srcs * kECTblBytes;
#define LIZEC_LAUNCH_VIEW(SAL, DAL)                                         \
	hipLaunchKernelGGL(HIP_KERNEL_NAME(ec_encode_view_kernel<D, CH, SAL, DAL>), \
	                   dim3(total_tiles), dim3(kThreads), lds, s, srcs,     \
	                   dest_base, v.tbls, v.index, v.map, v.view,           \
	                   v.view_parts, v.chunk_nb, v.row_cols, v.col0, v.dst, \
	                   v.dst_nb, dests_total, src_stride, dst_stride)
	if (sal && dal) LIZEC_LAUNCH_VIEW(true, true);
	else if (sal) LIZEC_LAUNCH_VIEW(true, false);
	else if (dal) LIZEC_LAUNCH_VIEW(false, true);
	else LIZEC_LAUNCH_VIEW(false, false);
#undef LIZEC_LAUNCH_VIEW
}

extern "C" int lizec_ec_encode_batch_view(
    lizec_engine *e, int srcs, int dests, const uint8_t *gftbls, int ntables,
    const uint32_t *tbl_index, const uint64_t *view_dptrs, int view_parts,
    const uint32_t *chunk_blocks, int row_cols, const uint32_t *src_col0,
    const uint64_t *dst_dptrs, const uint32_t *dst_nblocks, int num_stripes,
    uint32_t src_block_stride, uint32_t dst_block_stride, void *stream) {
	if (!e || !gftbls || !view_dptrs || !chunk_blocks || !dst_dptrs ||
	    !dst_nblocks)
		return LIZEC_EINVAL;
	if (srcs < 1 || srcs > 32 || dests < 1 || dests > 32 || num_stripes < 1)
		return LIZEC_EINVAL;
	if (view_parts < 1 || view_parts > 32 || row_cols < 1 || row_cols > 32 ||
	    srcs > row_cols)
		return LIZEC_EINVAL;
	if (ntables < 1 ||
	    (uint64_t)ntables * 32 * srcs * dests > (uint64_t)1 << 30)
		return LIZEC_EINVAL;
	if (src_block_stride < kECBlockBytes || dst_block_stride < kECBlockBytes)
		return LIZEC_EINVAL;
	if (tbl_index)
		for (int i = 0; i < num_stripes; ++i)
			if (tbl_index[i] >= (uint32_t)ntables) return LIZEC_EINVAL;
	size_t nview = (size_t)num_stripes * view_parts;
	size_t ndst = (size_t)num_stripes * dests;
	/* the source side's bits: the stride and the view addresses in use,
	 * those of the parts that hold at least one block of their chunk */
	uint64_t sbits = src_block_stride, dbits = dst_block_stride;
	for (int i = 0; i < num_stripes; ++i) {
		uint32_t n = chunk_blocks[i];
		if (n == 0 || n > 1048576u) return LIZEC_EINVAL;
		if (src_col0 && (uint64_t)src_col0[i] + srcs > (uint64_t)row_cols)
			return LIZEC_EINVAL;
		const uint64_t *vp = view_dptrs + (size_t)i * view_parts;
		for (uint32_t p = 0; p < (uint32_t)view_parts && p < n; ++p) {
			if (!vp[p]) return LIZEC_EINVAL;
			sbits |= vp[p];
		}
	}
	for (size_t i = 0; i < ndst; ++i) {
		if (dst_nblocks[i] > 32768u) return LIZEC_EINVAL;
		if (!dst_nblocks[i]) continue;
		if (!dst_dptrs[i]) return LIZEC_EINVAL;
		dbits |= dst_dptrs[i];
	}
	if ((sbits | dbits) & 3) return LIZEC_EINVAL;
	const bool sal = (sbits & 15) == 0, dal = (dbits & 15) == 0;
	int64_t entries =
	    lizec_ragged_block_map(dst_nblocks, dests, num_stripes, nullptr, 0);
	if (entries <= 0) return LIZEC_EINVAL;
	hipStream_t s = stream ? (hipStream_t)stream : e->stream;
	LIZEC_CHECK(hipSetDevice(e->device));

	/* the ragged call's scratch, with the chunk counts and first columns
	 * where it keeps the source counts; every section 16-byte aligned */
	auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
	size_t ntbl = (size_t)ntables * srcs * dests;   /* 32-byte tables */
	size_t o_index = up16(ntbl * kECTblBytes);
	size_t o_map = o_index + up16((size_t)num_stripes * 4);
	size_t o_cnb = o_map + up16((size_t)entries * 8);
	size_t o_col = o_cnb + up16((size_t)num_stripes * 4);
	size_t o_dnb = o_col + up16((size_t)num_stripes * 4);
	size_t bytes = o_dnb + up16(ndst * 4);
	lizec_stream_ctx *c;
	int r = ctx_acquire_ragged(e, s, nview + ndst, (nview + ndst) * 8, bytes,
	                           &c);
	if (r != LIZEC_OK) return r;
	uint8_t *h = c->h_ragged;
	for (size_t i = 0; i < ntbl; ++i)
		pack_mixed_radix(gftbls + i * 32, h + i * kECTblBytes);
	if (tbl_index)
		memcpy(h + o_index, tbl_index, (size_t)num_stripes * 4);
	else
		memset(h + o_index, 0, (size_t)num_stripes * 4);
	if (lizec_ragged_block_map(dst_nblocks, dests, num_stripes,
	                           (uint32_t *)(h + o_map),
	                           (uint64_t)entries) != entries)
		return LIZEC_EINVAL;
	memcpy(h + o_cnb, chunk_blocks, (size_t)num_stripes * 4);
	if (src_col0)
		memcpy(h + o_col, src_col0, (size_t)num_stripes * 4);
	else
		memset(h + o_col, 0, (size_t)num_stripes * 4);
	memcpy(h + o_dnb, dst_nblocks, ndst * 4);
	uint64_t *pstage = (uint64_t *)(c->h_staging + (size_t)kECTblBytes * 32 * 32);
	memcpy(pstage, view_dptrs, nview * 8);
	memcpy(pstage + nview, dst_dptrs, ndst * 8);
	LIZEC_CHECK(hipMemcpyAsync(c->d_ragged, h, bytes, hipMemcpyHostToDevice, s));
	LIZEC_CHECK(hipMemcpyAsync(c->d_ptrs, pstage, (nview + ndst) * 8,
	                           hipMemcpyHostToDevice, s));
	LIZEC_CHECK(hipEventRecord(c->uploaded, s));
	c->ev_recorded = true;

	view_dev vd;
	vd.tbls = c->d_ragged;
	vd.index = (const uint32_t *)(c->d_ragged + o_index);
	vd.map = (const uint2 *)(c->d_ragged + o_map);
	vd.chunk_nb = (const uint32_t *)(c->d_ragged + o_cnb);
	vd.col0 = (const uint32_t *)(c->d_ragged + o_col);
	vd.dst_nb = (const uint32_t *)(c->d_ragged + o_dnb);
	vd.view = c->d_ptrs;
	vd.dst = c->d_ptrs + nview;
	vd.view_parts = (uint32_t)view_parts;
	vd.row_cols = (uint32_t)row_cols;
	/* passes of at most 8 destinations, as run_batch_strided */
	for (int base = 0; base < dests;) {
		int d = dests - base;
		if (d > 8) d = 8;
#define LIZEC_LAUNCH_VIEW_D(D)                                             \
	launch_ec_view<D>((uint32_t)entries, srcs, base, vd, dests,            \
	                  src_block_stride, dst_block_stride, sal, dal, s)
		switch (d) {
		case 1: LIZEC_LAUNCH_VIEW_D(1); break;
		case 2: LIZEC_LAUNCH_VIEW_D(2); break;
		case 3: LIZEC_LAUNCH_VIEW_D(3); break;
		case 4: LIZEC_LAUNCH_VIEW_D(4); break;
		case 5: LIZEC_LAUNCH_VIEW_D(5); break;
		case 6: LIZEC_LAUNCH_VIEW_D(6); break;
		case 7: LIZEC_LAUNCH_VIEW_D(7); break;
		default: LIZEC_LAUNCH_VIEW_D(8); break;
		}
#undef LIZEC_LAUNCH_VIEW_D
		base += d;
	}
	LIZEC_CHECK(hipGetLastError());
	return LIZEC_OK;
}

/* ------------------------------------------------------------------ */
/* Chunk reads: block ranges gathered from the parts of a slice, lost  */
/* parts rebuilt on the way (ec_kernel_read.h)                         */
/* ------------------------------------------------------------------ */

struct read_dev {
	const uint8_t *tbls;
	const uint32_t *index;
	const uint2 *map;
	const uint64_t *src, *dst;
	const uint32_t *src_nb, *slot_col, *row_col;
	const uint2 *range;
	uint32_t view_parts;
};

/* One pass of the read kernel: the grid of launch_ec_ragged.  D = 0 is the
 * pure gather and needs no LDS. */
template <int D>
static void launch_chunk_read(uint32_t entries, int srcs, int dest_base,
                              int rows, const read_dev &r, uint32_t src_stride,
                              uint32_t dst_stride, bool sal, bool dal,
                              hipStream_t s) {
	constexpr int CH = ec_chunks_for(D);
	uint32_t total_tiles = entries * (kECBlockBytes / (kChunkBytes * CH));
	size_t lds = (size_t)D * srcs * kECTblBytes;
#define LIZEC_LAUNCH_READ(SAL, DAL)                                         \
	hipLaunchKernelGGL(HIP_KERNEL_NAME(ec_chunk_read_kernel<D, CH, SAL, DAL>), \
	                   dim3(total_tiles), dim3(kThreads), lds, s, srcs,     \
	                   dest_base, rows, r.tbls, r.index, r.map, r.src,      \
	                   r.src_nb, r.slot_col, r.row_col, r.view_parts,       \
	                   r.range, r.dst, src_stride, dst_stride)
	if (sal && dal) LIZEC_LAUNCH_READ(true, true);
	else if (sal) LIZEC_LAUNCH_READ(true, false);
	else if (dal) LIZEC_LAUNCH_READ(false, true);
	else LIZEC_LAUNCH_READ(false, false);
#undef LIZEC_LAUNCH_READ
}

extern "C" int64_t lizec_impl_chunk_read_check(
    int srcs, int rows, const uint8_t *gftbls, int ntables,
    const uint32_t *tbl_index, const uint64_t *src_dptrs,
    const uint32_t *src_nblocks, int view_parts, const uint8_t *col_map,
    const uint32_t *first_block, const uint32_t *block_count,
    const uint64_t *dst_dptrs, int num_reads, uint32_t src_block_stride,
    uint32_t dst_block_stride, uint64_t *sbits_out, uint64_t *dbits_out);

/* The body of lizec_chunk_read_batch and lizec_chunk_read_verified_batch.
 * With crc_dptrs the sources are checked first (read_verify.h): dev_bad is
 * zeroed, the verify kernel runs, then the launches of the plain read. */
static int chunk_read_run(
    lizec_engine *e, int srcs, int rows, const uint8_t *gftbls, int ntables,
    const uint32_t *tbl_index, const uint64_t *src_dptrs,
    const uint32_t *src_nblocks, int view_parts, const uint8_t *col_map,
    const uint32_t *first_block, const uint32_t *block_count,
    const uint64_t *dst_dptrs, int num_reads, uint32_t src_block_stride,
    uint32_t dst_block_stride, const uint64_t *crc_dptrs,
    uint32_t crc_block_stride, uint32_t *dev_bad, void *stream) {
	if (!e) return LIZEC_EINVAL;
	uint64_t sbits, dbits;
	int64_t entries = lizec_impl_chunk_read_check(
	    srcs, rows, gftbls, ntables, tbl_index, src_dptrs, src_nblocks,
	    view_parts, col_map, first_block, block_count, dst_dptrs, num_reads,
	    src_block_stride, dst_block_stride, &sbits, &dbits);
	if (entries <= 0) return LIZEC_EINVAL;
	const bool sal = (sbits & 15) == 0, dal = (dbits & 15) == 0;
	hipStream_t s = stream ? (hipStream_t)stream : e->stream;
	LIZEC_CHECK(hipSetDevice(e->device));

	/* the ragged call's scratch with the read's own tables in place of the
	 * destination counts; every section 16-byte aligned */
	auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
	const size_t R = (size_t)num_reads, ks = (size_t)view_parts;
	const size_t nsrc = R * srcs, nrow = R * rows;
	size_t ntbl = rows ? (size_t)ntables * srcs * rows : 0;   /* 32 B each */
	size_t o_index = up16(ntbl * kECTblBytes);
	size_t o_map = o_index + up16(R * 4);
	size_t o_snb = o_map + up16((size_t)entries * 8);
	size_t o_scol = o_snb + up16(nsrc * 4);
	size_t o_rcol = o_scol + up16(nsrc * 4);
	size_t o_range = o_rcol + up16(nrow * 4);
	size_t bytes = o_range + up16(R * 8);
	lizec_stream_ctx *c;
	/* a verified read stages the CRC addresses behind the destinations */
	const size_t nptr = nsrc + R + (crc_dptrs ? nsrc : 0);
	int r = ctx_acquire_ragged(e, s, nptr, nptr * 8, bytes, &c);
	if (r != LIZEC_OK) return r;
	if (crc_dptrs) LIZEC_CHECK(hipMemsetAsync(dev_bad, 0, R * 4, s));
	uint8_t *h = c->h_ragged;
	for (size_t i = 0; i < ntbl; ++i)
		pack_mixed_radix(gftbls + i * 32, h + i * kECTblBytes);
	if (rows && tbl_index)
		memcpy(h + o_index, tbl_index, R * 4);
	else
		memset(h + o_index, 0, R * 4);
	/* the row map, and the two inverses of col_map: the column a slot backs
	 * and the column a table row stands for */
	uint32_t *map = (uint32_t *)(h + o_map);
	uint32_t *scol = (uint32_t *)(h + o_scol);
	uint32_t *rcol = (uint32_t *)(h + o_rcol);
	uint32_t *range = (uint32_t *)(h + o_range);
	memset(scol, 0xFF, nsrc * 4);
	memset(rcol, 0xFF, nrow * 4);
	for (size_t i = 0; i < R; ++i) {
		const uint32_t first = first_block[i];
		const uint32_t last = first + block_count[i] - 1;
		for (uint32_t b = first / (uint32_t)ks; b <= last / (uint32_t)ks; ++b) {
			*map++ = (uint32_t)i;
			*map++ = b;
		}
		for (size_t col = 0; col < ks; ++col) {
			const uint8_t v = col_map[i * ks + col];
			if (v == 0xFF) continue;
			if (v >= 0x80) rcol[i * rows + (v - 0x80)] = (uint32_t)col;
			else scol[i * srcs + v] = (uint32_t)col;
		}
		range[2 * i] = first;
		range[2 * i + 1] = block_count[i];
	}
	memcpy(h + o_snb, src_nblocks, nsrc * 4);
	uint64_t *pstage = (uint64_t *)(c->h_staging + (size_t)kECTblBytes * 32 * 32);
	memcpy(pstage, src_dptrs, nsrc * 8);
	memcpy(pstage + nsrc, dst_dptrs, R * 8);
	if (crc_dptrs) memcpy(pstage + nsrc + R, crc_dptrs, nsrc * 8);
	LIZEC_CHECK(hipMemcpyAsync(c->d_ragged, h, bytes, hipMemcpyHostToDevice, s));
	LIZEC_CHECK(hipMemcpyAsync(c->d_ptrs, pstage, nptr * 8,
	                           hipMemcpyHostToDevice, s));
	LIZEC_CHECK(hipEventRecord(c->uploaded, s));
	c->ev_recorded = true;

	read_dev rd;
	rd.tbls = c->d_ragged;
	rd.index = (const uint32_t *)(c->d_ragged + o_index);
	rd.map = (const uint2 *)(c->d_ragged + o_map);
	rd.src_nb = (const uint32_t *)(c->d_ragged + o_snb);
	rd.slot_col = (const uint32_t *)(c->d_ragged + o_scol);
	rd.row_col = (const uint32_t *)(c->d_ragged + o_rcol);
	rd.range = (const uint2 *)(c->d_ragged + o_range);
	rd.src = c->d_ptrs;
	rd.dst = c->d_ptrs + nsrc;
	rd.view_parts = (uint32_t)view_parts;
	if (crc_dptrs) {
		/* one wave per (map entry, slot), four per workgroup: at most
		 * entries * 8 workgroups, which the check bounds by 2^31 - 1 */
		const uint64_t items = (uint64_t)entries * srcs;
		hipLaunchKernelGGL(chunk_read_verify_kernel,
		                   dim3((uint32_t)((items + 3) / 4)),
		                   dim3(kCrcRangesThreads), 0, s, srcs, rows, items,
		                   rd.map, rd.src, c->d_ptrs + nsrc + R, rd.src_nb,
		                   rd.slot_col, rd.row_col, rd.view_parts, rd.range,
		                   src_block_stride, crc_block_stride, e->d_crc_const,
		                   e->d_crc_const + kCrcTabWords, dev_bad);
	}
	/* passes of at most 8 table rows, as run_batch_strided; pass 0 copies */
	if (rows == 0)
		launch_chunk_read<0>((uint32_t)entries, srcs, 0, 0, rd,
		                     src_block_stride, dst_block_stride, sal, dal, s);
	for (int base = 0; base < rows;) {
		int d = rows - base;
		if (d > 8) d = 8;
#define LIZEC_LAUNCH_READ_D(D)                                             \
	launch_chunk_read<D>((uint32_t)entries, srcs, base, rows, rd,          \
	                     src_block_stride, dst_block_stride, sal, dal, s)
		switch (d) {
		case 1: LIZEC_LAUNCH_READ_D(1); break;
		case 2: LIZEC_LAUNCH_READ_D(2); break;
		case 3: LIZEC_LAUNCH_READ_D(3); break;
		case 4: LIZEC_LAUNCH_READ_D(4); break;
		case 5: LIZEC_LAUNCH_READ_D(5); break;
		case 6: LIZEC_LAUNCH_READ_D(6); break;
		case 7: LIZEC_LAUNCH_READ_D(7); break;
		default: LIZEC_LAUNCH_READ_D(8); break;
		}
#undef LIZEC_LAUNCH_READ_D
		base += d;
	}
	LIZEC_CHECK(hipGetLastError());
	return LIZEC_OK;
}

extern "C" int lizec_chunk_read_batch(
    lizec_engine *e, int srcs, int rows, const uint8_t *gftbls, int ntables,
    const uint32_t *tbl_index, const uint64_t *src_dptrs,
    const uint32_t *src_nblocks, int view_parts, const uint8_t *col_map,
    const uint32_t *first_block, const uint32_t *block_count,
    const uint64_t *dst_dptrs, int num_reads, uint32_t src_block_stride,
    uint32_t dst_block_stride, void *stream) {
	return chunk_read_run(e, srcs, rows, gftbls, ntables, tbl_index, src_dptrs,
	                      src_nblocks, view_parts, col_map, first_block,
	                      block_count, dst_dptrs, num_reads, src_block_stride,
	                      dst_block_stride, nullptr, 0, nullptr, stream);
}

extern "C" int lizec_chunk_read_verified_batch(
    lizec_engine *e, int srcs, int rows, const uint8_t *gftbls, int ntables,
    const uint32_t *tbl_index, const uint64_t *src_dptrs,
    const uint32_t *src_nblocks, int view_parts, const uint8_t *col_map,
    const uint32_t *first_block, const uint32_t *block_count,
    const uint64_t *dst_dptrs, int num_reads, uint32_t src_block_stride,
    uint32_t dst_block_stride, const uint64_t *crc_dptrs,
    uint32_t crc_block_stride, uint32_t *dev_bad_out, void *stream) {
	if (!crc_dptrs || !dev_bad_out || crc_block_stride < 4) return LIZEC_EINVAL;
	return chunk_read_run(e, srcs, rows, gftbls, ntables, tbl_index, src_dptrs,
	                      src_nblocks, view_parts, col_map, first_block,
	                      block_count, dst_dptrs, num_reads, src_block_stride,
	                      dst_block_stride, crc_dptrs, crc_block_stride,
	                      dev_bad_out, stream);
}

/* Multi-table launch: same grid/tile/LDS shape as launch_ec. */
template <int D>
static void launch_ec_multi(uint32_t part_len, int srcs, int dest_base,
                            const uint8_t *d_tbls, const uint32_t *d_index,
                            const uint64_t *d_src, const uint64_t *d_dst,
                            int dests_total, uint32_t nstripes,
                            hipStream_t s) {
	constexpr int CH = ec_chunks_for(D);
	uint32_t tile_bytes = kChunkBytes * CH;
	uint32_t tiles_per_part = (part_len + tile_bytes - 1) / tile_bytes;
	uint32_t total_tiles = tiles_per_part * nstripes;
	uint32_t grid = total_tiles < 1048576u ? total_tiles : 1048576u;
	size_t lds = (size_t)D * srcs * kECTblBytes;
	hipLaunchKernelGGL(HIP_KERNEL_NAME(ec_encode_multi_kernel<D, CH, kECSwz, kECNtStore, kECNtLoad>),
	                   dim3(grid), dim3(kThreads), lds, s,
	                   part_len, srcs, dest_base, d_tbls, d_index, d_src,
	                   d_dst, dests_total, tiles_per_part, total_tiles);
}

/* run_batch for per-stripe tables: the same split into passes of at most 8
 * destinations; dest_base then offsets into every stripe's own table. */
static int run_batch_multi(uint64_t part_len, int srcs, int dests,
                           const uint8_t *d_tbls, const uint32_t *d_index,
                           const uint64_t *d_src, const uint64_t *d_dst,
                           uint32_t num_stripes, hipStream_t s) {
	for (int base = 0; base < dests;) {
		int d = dests - base;
		if (d > 8) d = 8;
#define LIZEC_LAUNCH_MULTI(D)                                              \
	launch_ec_multi<D>((uint32_t)part_len, srcs, base, d_tbls, d_index,    \
	                   d_src, d_dst, dests, num_stripes, s)
		switch (d) {
		case 1: LIZEC_LAUNCH_MULTI(1); break;
		case 2: LIZEC_LAUNCH_MULTI(2); break;
		case 3: LIZEC_LAUNCH_MULTI(3); break;
		case 4: LIZEC_LAUNCH_MULTI(4); break;
		case 5: LIZEC_LAUNCH_MULTI(5); break;
		case 6: LIZEC_LAUNCH_MULTI(6); break;
		case 7: LIZEC_LAUNCH_MULTI(7); break;
		default: LIZEC_LAUNCH_MULTI(8); break;
		}
#undef LIZEC_LAUNCH_MULTI
		base += d;
	}
	LIZEC_CHECK(hipGetLastError());
	return LIZEC_OK;
}

/* check_batch_args plus the multi-table rules; runs entirely on the host,
 * before anything is allocated or enqueued. */
static int check_multi_args(uint64_t part_len, int srcs, int dests,
                            const uint8_t *gftbls, int ntables,
                            const uint32_t *tbl_index,
                            const uint64_t *src_dptrs,
                            const uint64_t *dst_dptrs, int num_stripes) {
	int r = check_batch_args(part_len, srcs, dests, num_stripes);
	if (r != LIZEC_OK) return r;
	if (!gftbls || !tbl_index || !src_dptrs || !dst_dptrs) return LIZEC_EINVAL;
	if (ntables < 1 ||
	    (uint64_t)ntables * 32 * srcs * dests > (uint64_t)1 << 30)
		return LIZEC_EINVAL;
	for (int i = 0; i < num_stripes; ++i)
		if (tbl_index[i] >= (uint32_t)ntables) return LIZEC_EINVAL;
	return check_part_addrs(src_dptrs, (size_t)num_stripes * srcs, dst_dptrs,
	                        (size_t)num_stripes * dests);
}

extern "C" int lizec_ec_encode_batch_multi(lizec_engine *e, uint64_t part_len,
                                           int srcs, int dests,
                                           const uint8_t *gftbls, int ntables,
                                           const uint32_t *tbl_index,
                                           const uint64_t *src_dptrs,
                                           const uint64_t *dst_dptrs,
                                           int num_stripes, void *stream) {
	if (!e) return LIZEC_EINVAL;
	int r = check_multi_args(part_len, srcs, dests, gftbls, ntables,
	                         tbl_index, src_dptrs, dst_dptrs, num_stripes);
	if (r != LIZEC_OK) return r;
	hipStream_t s = stream ? (hipStream_t)stream : e->stream;
	LIZEC_CHECK(hipSetDevice(e->device));

	size_t nsrc = (size_t)num_stripes * srcs;
	size_t ndst = (size_t)num_stripes * dests;
	size_t ntbl = (size_t)ntables * srcs * dests;   /* 32-byte tables */
	size_t tbl_bytes = ntbl * kECTblBytes;
	lizec_stream_ctx *c;
	r = ctx_acquire_multi(e, s, nsrc + ndst, (nsrc + ndst) * 8, tbl_bytes,
	                      (size_t)num_stripes, &c);
	if (r != LIZEC_OK) return r;
	uint64_t *d_src = c->d_ptrs;
	uint64_t *d_dst = c->d_ptrs + nsrc;
	/* pointer arrays go through the shared staging buffer (past its
	 * single-table area), tables + index through the multi one */
	uint64_t *pstage = (uint64_t *)(c->h_staging + (size_t)kECTblBytes * 32 * 32);
	uint8_t *tstage = c->h_mstaging;
	uint32_t *istage = (uint32_t *)(c->h_mstaging + tbl_bytes);
	for (size_t i = 0; i < ntbl; ++i)
		pack_mixed_radix(gftbls + i * 32, tstage + i * kECTblBytes);
	memcpy(istage, tbl_index, (size_t)num_stripes * 4);
	memcpy(pstage, src_dptrs, nsrc * 8);
	memcpy(pstage + nsrc, dst_dptrs, ndst * 8);
	LIZEC_CHECK(hipMemcpyAsync(c->d_mtbls, tstage, tbl_bytes,
	                           hipMemcpyHostToDevice, s));
	LIZEC_CHECK(hipMemcpyAsync(c->d_mindex, istage, (size_t)num_stripes * 4,
	                           hipMemcpyHostToDevice, s));
	LIZEC_CHECK(hipMemcpyAsync(d_src, pstage, (nsrc + ndst) * 8,
	                           hipMemcpyHostToDevice, s));
	LIZEC_CHECK(hipEventRecord(c->uploaded, s));
	c->ev_recorded = true;

	return run_batch_multi(part_len, srcs, dests, c->d_mtbls, c->d_mindex,
	                       d_src, d_dst, (uint32_t)num_stripes, s);
}

extern "C" int lizec_ec_plan_create_multi(lizec_engine *e, uint64_t part_len,
                                          int srcs, int dests,
                                          const uint8_t *gftbls, int ntables,
                                          const uint32_t *tbl_index,
                                          const uint64_t *src_dptrs,
                                          const uint64_t *dst_dptrs,
                                          int num_stripes, lizec_plan **out) {
	*out = nullptr;
	if (!e) return LIZEC_EINVAL;
	int r = check_multi_args(part_len, srcs, dests, gftbls, ntables,
	                         tbl_index, src_dptrs, dst_dptrs, num_stripes);
	if (r != LIZEC_OK) return r;
	LIZEC_CHECK(hipSetDevice(e->device));
	size_t nsrc = (size_t)num_stripes * srcs;
	size_t ndst = (size_t)num_stripes * dests;
	size_t ntbl = (size_t)ntables * srcs * dests;
	size_t tbl_bytes = ntbl * kECTblBytes;
	uint8_t *packed = (uint8_t *)malloc(tbl_bytes);
	if (!packed) return LIZEC_ENOMEM;
	for (size_t i = 0; i < ntbl; ++i)
		pack_mixed_radix(gftbls + i * 32, packed + i * kECTblBytes);
	lizec_plan *p = new lizec_plan();
	p->e = e;
	p->part_len = part_len;
	p->srcs = srcs;
	p->dests = dests;
	p->num_stripes = num_stripes;
	if (hipMalloc(&p->d_tbls, tbl_bytes) != hipSuccess ||
	    hipMalloc(&p->d_src, nsrc * 8) != hipSuccess ||
	    hipMalloc(&p->d_dst, ndst * 8) != hipSuccess ||
	    hipMalloc(&p->d_index, (size_t)num_stripes * 4) != hipSuccess) {
		free(packed);
		lizec_ec_plan_destroy(p);
		return LIZEC_ENOMEM;
	}
	bool ok = hipMemcpy(p->d_tbls, packed, tbl_bytes,
	                    hipMemcpyHostToDevice) == hipSuccess &&
	          hipMemcpy(p->d_index, tbl_index, (size_t)num_stripes * 4,
	                    hipMemcpyHostToDevice) == hipSuccess &&
	          hipMemcpy(p->d_src, src_dptrs, nsrc * 8,
	                    hipMemcpyHostToDevice) == hipSuccess &&
	          hipMemcpy(p->d_dst, dst_dptrs, ndst * 8,
	                    hipMemcpyHostToDevice) == hipSuccess;
	free(packed);
	if (!ok) {
		lizec_ec_plan_destroy(p);
		return LIZEC_EHIP;
	}
	*out = p;
	return LIZEC_OK;
}

extern "C" int lizec_ec_plan_create(lizec_engine *e, uint64_t part_len,
                                    int srcs, int dests,
                                    const uint8_t *gftbls,
                                    const uint64_t *src_dptrs,
                                    const uint64_t *dst_dptrs,
                                    int num_stripes, lizec_plan **out) {
	*out = nullptr;
	if (!e) return LIZEC_EINVAL;
	int r = check_batch_args(part_len, srcs, dests, num_stripes);
	if (r != LIZEC_OK) return r;
	size_t nsrc = (size_t)num_stripes * srcs;
	size_t ndst = (size_t)num_stripes * dests;
	r = check_part_addrs(src_dptrs, nsrc, dst_dptrs, ndst);
	if (r != LIZEC_OK) return r;
	LIZEC_CHECK(hipSetDevice(e->device));
	lizec_plan *p = new lizec_plan();
	p->e = e;
	p->part_len = part_len;
	p->srcs = srcs;
	p->dests = dests;
	p->num_stripes = num_stripes;
	if (hipMalloc(&p->d_tbls, (size_t)kECTblBytes * srcs * dests) != hipSuccess ||
	    hipMalloc(&p->d_src, nsrc * 8) != hipSuccess ||
	    hipMalloc(&p->d_dst, ndst * 8) != hipSuccess) {
		lizec_ec_plan_destroy(p);
		return LIZEC_ENOMEM;
	}
	uint8_t packed[kECTblBytes * 32 * 32];
	for (int i = 0; i < srcs * dests; ++i)
		pack_mixed_radix(gftbls + (size_t)i * 32, packed + (size_t)i * kECTblBytes);
	if (hipMemcpy(p->d_tbls, packed, (size_t)kECTblBytes * srcs * dests,
	              hipMemcpyHostToDevice) != hipSuccess ||
	    hipMemcpy(p->d_src, src_dptrs, nsrc * 8,
	              hipMemcpyHostToDevice) != hipSuccess ||
	    hipMemcpy(p->d_dst, dst_dptrs, ndst * 8,
	              hipMemcpyHostToDevice) != hipSuccess) {
		lizec_ec_plan_destroy(p);
		return LIZEC_EHIP;
	}
	*out = p;
	return LIZEC_OK;
}

extern "C" int lizec_ec_plan_run(lizec_plan *p, void *stream) {
	if (!p) return LIZEC_EINVAL;
	hipStream_t s = stream ? (hipStream_t)stream : p->e->stream;
	LIZEC_CHECK(hipSetDevice(p->e->device));
	if (p->d_index)
		return run_batch_multi(p->part_len, p->srcs, p->dests, p->d_tbls,
		                       p->d_index, p->d_src, p->d_dst,
		                       (uint32_t)p->num_stripes, s);
	return run_batch(p->part_len, p->srcs, p->dests, p->d_tbls, p->d_src,
	                 p->d_dst, (uint32_t)p->num_stripes, s);
}

extern "C" void lizec_ec_plan_destroy(lizec_plan *p) {
	if (!p) return;
	(void)hipFree(p->d_tbls);
	(void)hipFree(p->d_src);
	(void)hipFree(p->d_dst);
	(void)hipFree(p->d_index);
	delete p;
}

extern "C" int lizec_crc32_batch(lizec_engine *e, const void *dev_buf,
                                 uint32_t block_len, uint64_t nblocks,
                                 uint32_t seed, uint32_t *dev_crcs_out,
                                 void *stream) {
	if (!e || !dev_buf || !dev_crcs_out || nblocks < 1) return LIZEC_EINVAL;
	/* one wave per block, 64 equal lane segments, 16B vector loads */
	if (block_len == 0 || (block_len & 1023)) return LIZEC_EINVAL;
	/* The matrix bank holds M_0..M_{kCrcMatCount-1}, so crc_advance can
	 * append any zero run shorter than 2^kCrcMatCount bytes.  The longest
	 * run a kernel asks for is block_len / 2: the last step of the shfl
	 * tree advances by 32 lane segments (32 * span / 64 = span / 2, with
	 * span = block_len / C), and the span splice of a C-chain kernel by
	 * span = block_len / C <= block_len / 2.  Hence block_len / 2 <
	 * 2^kCrcMatCount, i.e. block_len < 2^27; a longer block would index
	 * past the bank and return a wrong CRC. */
	if (block_len >= (2u << kCrcMatCount)) return LIZEC_EINVAL;
	/* every kernel reads the buffer in 32-bit words or wider */
	if ((uintptr_t)dev_buf & 3) return LIZEC_EINVAL;
	hipStream_t s = stream ? (hipStream_t)stream : e->stream;
	LIZEC_CHECK(hipSetDevice(e->device));
	uint64_t groups = (nblocks + 3) / 4;
	uint32_t grid = (uint32_t)(groups < 131072 ? groups : 131072);
	const char *ch = getenv("LIZEC_CRC_CHAINS");   /* A/B hooks */
	const char *sl = getenv("LIZEC_CRC_SLICE");
	const char *im = getenv("LIZEC_CRC_IMPL");
	const char *fn = getenv("LIZEC_CRC_FOLD_NACC");
	const char *nt = getenv("LIZEC_CRC_NT");
	const char *pf = getenv("LIZEC_CRC_PF");
	/* fold C=1 NACC=1 measured best (r2b: 5112 GB/s = 0.64 of spec peak
	 * vs table 3511; NT loads defeat the L1 line-burst reuse, -57%) */
	int chains = ch ? atoi(ch) : 1;
	int slice = sl ? atoi(sl) : 8;   /* slice-16 measured -16% within-box (profiles) */
	bool fold = !(im && strcmp(im, "table") == 0);
	int nacc = fn ? atoi(fn) : 1;
	bool ntld = nt && atoi(nt) != 0;
	/* burst prefetch measured box-DEPENDENT: +7% on one box (r2d,
	 * 5147 GB/s) but -20% on another (r2e, 4154 vs 5197 no-PF) — its
	 * 2-waves/SIMD occupancy is fragile, the 5-wave no-PF shape is
	 * robust across boxes.  Default off; env opt-in for A/B. */
	bool pfld = pf && atoi(pf) != 0;
	bool al16 = (((uintptr_t)dev_buf | block_len) & 15) == 0;
	/* A base that is 4- but not 16-byte aligned (the INTERLEAVED chunk
	 * format) may only reach kernels that load dwords: the fold kernels'
	 * AL16=false forms where the block splits into whole bursts, the
	 * generic kernel's otherwise.  The slicing kernels below load 16-byte
	 * vectors whatever the base. */
	if (!al16 && (!fold || block_len % (64 * 16 * 8) != 0)) {
		hipLaunchKernelGGL(HIP_KERNEL_NAME(crc32_blocks_kernel<false>),
		                   dim3(grid), dim3(kThreads), 0, s,
		                   (const uint8_t *)dev_buf, block_len, nblocks,
		                   seed, e->d_crc_const, dev_crcs_out);
		LIZEC_CHECK(hipGetLastError());
		return LIZEC_OK;
	}
	/* ...and the fold kernels have dword forms for one chain, and for two
	 * where the block splits into two spans of whole bursts */
	if (!al16 && !(chains == 2 && block_len % (2 * 64 * 16 * 8) == 0))
		chains = 1;
	/* carry-less-folding path (default): block must split into C spans of
	 * whole 64-lane x BV*16-byte bursts (BV=8) */
	if (fold && block_len % ((uint32_t)chains * 64 * 16 * 8) == 0 &&
	    (chains == 1 || chains == 2)) {
		const uint8_t *b = (const uint8_t *)dev_buf;
#define LIZEC_LAUNCH_FOLD(C, N, A, NT)                                       \
	hipLaunchKernelGGL(HIP_KERNEL_NAME(crc32_blocks_kernel_fold<C, N, A, NT>), \
	                   dim3(grid), dim3(kThreads), 0, s, b, block_len,       \
	                   nblocks, seed, e->d_crc_const, dev_crcs_out)
		if (!al16) {
			if (chains == 2) LIZEC_LAUNCH_FOLD(2, 2, false, false);
			else LIZEC_LAUNCH_FOLD(1, 1, false, false);
		} else if (chains == 2) {
			if (nacc == 1) LIZEC_LAUNCH_FOLD(2, 1, true, false);
			else LIZEC_LAUNCH_FOLD(2, 2, true, false);
		} else if (pfld) {
			const char *bv = getenv("LIZEC_CRC_BV");
			if (bv && atoi(bv) == 4)
				hipLaunchKernelGGL(HIP_KERNEL_NAME(crc32_blocks_kernel_fold<1, 1, true, false, true, 4>),
				                   dim3(grid), dim3(kThreads), 0, s, b,
				                   block_len, nblocks, seed, e->d_crc_const,
				                   dev_crcs_out);
			else
				hipLaunchKernelGGL(HIP_KERNEL_NAME(crc32_blocks_kernel_fold<1, 1, true, false, true>),
				                   dim3(grid), dim3(kThreads), 0, s, b,
				                   block_len, nblocks, seed, e->d_crc_const,
				                   dev_crcs_out);
		} else if (ntld) {
			if (nacc == 1) LIZEC_LAUNCH_FOLD(1, 1, true, true);
			else if (nacc == 4) LIZEC_LAUNCH_FOLD(1, 4, true, true);
			else LIZEC_LAUNCH_FOLD(1, 2, true, true);
		} else {
			const char *bv = getenv("LIZEC_CRC_BV");
			const char *at = getenv("LIZEC_CRC_AUTOTUNE");
			bool tune = !(at && atoi(at) == 0);
			if (bv && atoi(bv) == 4 && nacc == 1) {
				hipLaunchKernelGGL(HIP_KERNEL_NAME(crc32_blocks_kernel_fold<1, 1, true, false, false, 4>),
				                   dim3(grid), dim3(kThreads), 0, s, b,
				                   block_len, nblocks, seed, e->d_crc_const,
				                   dev_crcs_out);
			} else if (nacc == 4) {
				if (bv && atoi(bv) == 4)
					hipLaunchKernelGGL(HIP_KERNEL_NAME(crc32_blocks_kernel_fold<1, 4, true, false, false, 4>),
					                   dim3(grid), dim3(kThreads), 0, s, b,
					                   block_len, nblocks, seed,
					                   e->d_crc_const, dev_crcs_out);
				else
					LIZEC_LAUNCH_FOLD(1, 4, true, false);
			} else if (nacc == 2) {
				if (bv && atoi(bv) == 4)
					hipLaunchKernelGGL(HIP_KERNEL_NAME(crc32_blocks_kernel_fold<1, 2, true, false, false, 4>),
					                   dim3(grid), dim3(kThreads), 0, s, b,
					                   block_len, nblocks, seed,
					                   e->d_crc_const, dev_crcs_out);
				else
					LIZEC_LAUNCH_FOLD(1, 2, true, false);
			} else {
				int shape = e->crc_shape.load(std::memory_order_relaxed);
				if (shape < 0 && tune && nblocks >= 4096) {
					/* Autotune once per engine: time both shapes on this
					 * batch.  Both kernels emit the correct CRCs, so the
					 * probe costs one extra pass and the call stays
					 * correct even if timing fails. */
					hipEvent_t ev[3];
					int made = 0;
					for (; made < 3; ++made)
						if (hipEventCreate(&ev[made]) != hipSuccess) break;
					if (made == 3) {
						(void)hipEventRecord(ev[0], s);
						LIZEC_LAUNCH_FOLD(1, 1, true, false);
						(void)hipEventRecord(ev[1], s);
						hipLaunchKernelGGL(HIP_KERNEL_NAME(crc32_blocks_kernel_fold<1, 1, true, false, true>),
						                   dim3(grid), dim3(kThreads), 0, s,
						                   b, block_len, nblocks, seed,
						                   e->d_crc_const, dev_crcs_out);
						(void)hipEventRecord(ev[2], s);
						if (hipEventSynchronize(ev[2]) == hipSuccess) {
							float t0 = 0.f, t1 = 0.f;
							(void)hipEventElapsedTime(&t0, ev[0], ev[1]);
							(void)hipEventElapsedTime(&t1, ev[1], ev[2]);
							shape = (t1 > 0.f && t1 < t0) ? 1 : 0;
							e->crc_shape.store(shape,
							                   std::memory_order_relaxed);
						}
					} else {
						LIZEC_LAUNCH_FOLD(1, 1, true, false);
					}
					for (int i = 0; i < made; ++i)
						(void)hipEventDestroy(ev[i]);
					LIZEC_CHECK(hipGetLastError());
					return LIZEC_OK;
				}
				if (shape == 1)
					hipLaunchKernelGGL(HIP_KERNEL_NAME(crc32_blocks_kernel_fold<1, 1, true, false, true>),
					                   dim3(grid), dim3(kThreads), 0, s, b,
					                   block_len, nblocks, seed,
					                   e->d_crc_const, dev_crcs_out);
				else
					LIZEC_LAUNCH_FOLD(1, 1, true, false);
			}
		}
#undef LIZEC_LAUNCH_FOLD
		LIZEC_CHECK(hipGetLastError());
		return LIZEC_OK;
	}
	if (block_len % 32768 == 0 && chains >= 4)
		hipLaunchKernelGGL(HIP_KERNEL_NAME(crc32_blocks_kernel_multi<4, 8>),
		                   dim3(grid), dim3(kThreads), 0, s,
		                   (const uint8_t *)dev_buf, block_len, nblocks,
		                   seed, e->d_crc_const, dev_crcs_out);
	else if (block_len % 16384 == 0 && slice == 8)
		hipLaunchKernelGGL(HIP_KERNEL_NAME(crc32_blocks_kernel_multi<2, 8, 8>),
		                   dim3(grid), dim3(kThreads), 0, s,
		                   (const uint8_t *)dev_buf, block_len, nblocks,
		                   seed, e->d_crc_const, dev_crcs_out);
	else if (block_len % 16384 == 0)
		hipLaunchKernelGGL(HIP_KERNEL_NAME(crc32_blocks_kernel_multi<2, 8>),
		                   dim3(grid), dim3(kThreads), 0, s,
		                   (const uint8_t *)dev_buf, block_len, nblocks,
		                   seed, e->d_crc_const, dev_crcs_out);
	else
		hipLaunchKernelGGL(HIP_KERNEL_NAME(crc32_blocks_kernel<true>),
		                   dim3(grid), dim3(kThreads), 0, s,
		                   (const uint8_t *)dev_buf, block_len, nblocks,
		                   seed, e->d_crc_const, dev_crcs_out);
	LIZEC_CHECK(hipGetLastError());
	return LIZEC_OK;
}

/* ------------------------------------------------------------------ */
/* Byte-range CRC and the write gate (crc_ranges.h)                   */
/* ------------------------------------------------------------------ */

static_assert(kCrcRangesMats <= kCrcMatCount, "matrix bank too short");
static_assert(sizeof(lizec_write_op) == 40, "lizec_write_op has padding");

constexpr uint32_t kCrcRangesMaxN = 1u << 24;
constexpr uint32_t kCrcRangesMaxGrid = 16384;   /* x 4 waves (lizec.h) */

/* One wave per range over device-resident tables; d_nz = nullptr for the
 * plain form, else the per-range "holds a non-zero byte" words. */
static int launch_crc_ranges(lizec_engine *e, const uint64_t *d_addrs,
                             const uint32_t *d_lens, uint32_t n, uint32_t seed,
                             uint32_t *d_out, uint32_t *d_nz, hipStream_t s) {
	uint32_t groups = (n + 3) / 4;
	uint32_t grid = groups < kCrcRangesMaxGrid ? groups : kCrcRangesMaxGrid;
	if (d_nz)
		hipLaunchKernelGGL(HIP_KERNEL_NAME(crc32_ranges_kernel<true>),
		                   dim3(grid), dim3(kCrcRangesThreads), 0, s, d_addrs,
		                   d_lens, n, seed, e->d_crc_const,
		                   e->d_crc_const + kCrcTabWords, d_out, d_nz);
	else
		hipLaunchKernelGGL(HIP_KERNEL_NAME(crc32_ranges_kernel<false>),
		                   dim3(grid), dim3(kCrcRangesThreads), 0, s, d_addrs,
		                   d_lens, n, seed, e->d_crc_const,
		                   e->d_crc_const + kCrcTabWords, d_out, nullptr);
	LIZEC_CHECK(hipGetLastError());
	return LIZEC_OK;
}

extern "C" int lizec_crc32_ranges(lizec_engine *e, const uint64_t *dptrs,
                                  const uint32_t *lens, uint32_t n,
                                  uint32_t seed, uint32_t *dev_crcs_out,
                                  void *stream) {
	if (!e || !dptrs || !lens || !dev_crcs_out || n == 0 ||
	    n > kCrcRangesMaxN)
		return LIZEC_EINVAL;
	for (uint32_t i = 0; i < n; ++i)
		if (lens[i] > kCrcRangeMaxLen || (lens[i] && !dptrs[i]))
			return LIZEC_EINVAL;
	hipStream_t s = stream ? (hipStream_t)stream : e->stream;
	LIZEC_CHECK(hipSetDevice(e->device));
	/* scratch (u64 slots reused): [addrs u64 x n][lens u32 x n] */
	size_t slots = (size_t)n + ((size_t)n + 1) / 2;
	lizec_stream_ctx *c;
	int r = ctx_acquire(e, s, slots, slots * 8, &c);
	if (r != LIZEC_OK) return r;
	uint8_t *st = c->h_staging + (size_t)kECTblBytes * 32 * 32;
	memcpy(st, dptrs, (size_t)n * 8);
	memcpy(st + (size_t)n * 8, lens, (size_t)n * 4);
	LIZEC_CHECK(hipMemcpyAsync(c->d_ptrs, st, (size_t)n * 12,
	                           hipMemcpyHostToDevice, s));
	LIZEC_CHECK(hipEventRecord(c->uploaded, s));
	c->ev_recorded = true;
	return launch_crc_ranges(e, c->d_ptrs, (const uint32_t *)(c->d_ptrs + n), n,
	                         seed, dev_crcs_out, nullptr, s);
}

extern "C" int lizec_impl_write_gate_check(const lizec_write_op *ops,
                                           uint32_t n, uint32_t flags);

extern "C" int lizec_write_gate_batch(lizec_engine *e,
                                      const lizec_write_op *ops, uint32_t n,
                                      uint32_t flags, int32_t *dev_status_out,
                                      uint32_t *dev_newcrc_out, void *stream) {
	if (!e || !dev_status_out || !dev_newcrc_out) return LIZEC_EINVAL;
	int r = lizec_impl_write_gate_check(ops, n, flags);
	if (r != LIZEC_OK) return r;
	hipStream_t s = stream ? (hipStream_t)stream : e->stream;
	LIZEC_CHECK(hipSetDevice(e->device));
	/* scratch, in u64 slots: [ops 5n][range addrs 4n][range lens 2n] are
	 * uploaded; [range crcs 2n][range non-zero words 2n] are the ranges
	 * pass's outputs, read by the finishing kernel */
	const size_t N = n;
	lizec_stream_ctx *c;
	r = ctx_acquire(e, s, 15 * N, 11 * N * 8, &c);
	if (r != LIZEC_OK) return r;
	uint8_t *st = c->h_staging + (size_t)kECTblBytes * 32 * 32;
	memcpy(st, ops, N * sizeof(lizec_write_op));
	uint64_t *addrs = (uint64_t *)(st + 5 * N * 8);
	uint32_t *lens = (uint32_t *)(st + 9 * N * 8);
	for (size_t i = 0; i < N; ++i) {
		const lizec_write_op &op = ops[i];
		/* four slots per op: data, pre, changed, post; the block's three
		 * only for a partial write into an existing block */
		const bool blk =
		    op.block != 0 && !(op.offset == 0 && op.size == 65536u);
		const uint32_t end = op.offset + op.size;
		addrs[4 * i] = op.data;
		lens[4 * i] = op.size;
		addrs[4 * i + 1] = blk ? op.block : 0;
		lens[4 * i + 1] = blk ? op.offset : 0;
		addrs[4 * i + 2] = blk ? op.block + op.offset : 0;
		lens[4 * i + 2] = blk ? op.size : 0;
		addrs[4 * i + 3] = blk ? op.block + end : 0;
		lens[4 * i + 3] = blk ? 65536u - end : 0;
	}
	LIZEC_CHECK(hipMemcpyAsync(c->d_ptrs, st, 11 * N * 8,
	                           hipMemcpyHostToDevice, s));
	LIZEC_CHECK(hipEventRecord(c->uploaded, s));
	c->ev_recorded = true;
	const lizec_write_op *d_ops = (const lizec_write_op *)c->d_ptrs;
	const uint64_t *d_addrs = c->d_ptrs + 5 * N;
	const uint32_t *d_lens = (const uint32_t *)(c->d_ptrs + 9 * N);
	uint32_t *d_crcs = (uint32_t *)(c->d_ptrs + 11 * N);
	uint32_t *d_nz = (uint32_t *)(c->d_ptrs + 13 * N);
	r = launch_crc_ranges(e, d_addrs, d_lens, 4 * n, 0u, d_crcs, d_nz, s);
	if (r != LIZEC_OK) return r;
	hipLaunchKernelGGL(write_gate_finish_kernel,
	                   dim3((n + kCrcRangesThreads - 1) / kCrcRangesThreads),
	                   dim3(kCrcRangesThreads), 0, s, d_ops, n, flags, d_crcs,
	                   d_nz, e->d_crc_const + kCrcTabWords, dev_status_out,
	                   dev_newcrc_out);
	LIZEC_CHECK(hipGetLastError());
	return LIZEC_OK;
}

/* ------------------------------------------------------------------ */
/* The read gate (read_gate.h)                                        */
/* ------------------------------------------------------------------ */

static_assert(sizeof(lizec_read_op) == 32, "lizec_read_op has padding");

extern "C" int lizec_impl_read_gate_check(const lizec_read_op *ops, uint32_t n,
                                          uint32_t flags);

extern "C" int lizec_read_gate_batch(lizec_engine *e, const lizec_read_op *ops,
                                     uint32_t n, uint32_t flags,
                                     int32_t *dev_status_out, void *stream) {
	if (!e || !dev_status_out) return LIZEC_EINVAL;
	int r = lizec_impl_read_gate_check(ops, n, flags);
	if (r != LIZEC_OK) return r;
	hipStream_t s = stream ? (hipStream_t)stream : e->stream;
	LIZEC_CHECK(hipSetDevice(e->device));
	/* scratch, in u64 slots: [ops 4n], uploaded; the kernel needs no other */
	const size_t N = n;
	lizec_stream_ctx *c;
	r = ctx_acquire(e, s, 4 * N, N * sizeof(lizec_read_op), &c);
	if (r != LIZEC_OK) return r;
	uint8_t *st = c->h_staging + (size_t)kECTblBytes * 32 * 32;
	memcpy(st, ops, N * sizeof(lizec_read_op));
	LIZEC_CHECK(hipMemcpyAsync(c->d_ptrs, st, N * sizeof(lizec_read_op),
	                           hipMemcpyHostToDevice, s));
	LIZEC_CHECK(hipEventRecord(c->uploaded, s));
	c->ev_recorded = true;
	const lizec_read_op *d_ops = (const lizec_read_op *)c->d_ptrs;
	uint32_t groups = (n + 3) / 4;
	uint32_t grid = groups < kCrcRangesMaxGrid ? groups : kCrcRangesMaxGrid;
	if (flags & LIZEC_GATE_SPARSE)
		hipLaunchKernelGGL(HIP_KERNEL_NAME(read_gate_kernel<true>), dim3(grid),
		                   dim3(kCrcRangesThreads), 0, s, d_ops, n,
		                   e->d_crc_const, e->d_crc_const + kCrcTabWords,
		                   dev_status_out);
	else
		hipLaunchKernelGGL(HIP_KERNEL_NAME(read_gate_kernel<false>),
		                   dim3(grid), dim3(kCrcRangesThreads), 0, s, d_ops, n,
		                   e->d_crc_const, e->d_crc_const + kCrcTabWords,
		                   dev_status_out);
	LIZEC_CHECK(hipGetLastError());
	return LIZEC_OK;
}

/* ------------------------------------------------------------------ */
/* Chunk writes: parity of byte ranges written into a slice's blocks,  */
/* and the packets' CRCs (ec_kernel_write.h)                           */
/* ------------------------------------------------------------------ */

struct write_dev {
	const uint8_t *tbls;
	const uint4 *map16, *map8;   /* tile maps for 16 KiB / 8 KiB tiles */
	uint32_t tiles16, tiles8;
	const lizec_chunk_write *writes;
	const uint64_t *fill, *par;
	const uint32_t *fill_nb;
};

/* One pass of the write kernel: one workgroup per tile of the map that
 * matches the pass's tile size. */
template <int D>
static void launch_chunk_write(int ks, int dest_base, int rows,
                               const write_dev &w, uint32_t fill_stride,
                               bool fast, hipStream_t s) {
	constexpr int CH = ec_chunks_for(D);
	const uint32_t total_tiles = CH == 4 ? w.tiles16 : w.tiles8;
	const uint4 *map = CH == 4 ? w.map16 : w.map8;
	size_t lds = (size_t)D * ks * kECTblBytes;
#define LIZEC_LAUNCH_WRITE(FAST)                                            \
	hipLaunchKernelGGL(HIP_KERNEL_NAME(ec_chunk_write_kernel<D, CH, FAST>), \
	                   dim3(total_tiles), dim3(kThreads), lds, s, ks,       \
	                   dest_base, rows, w.tbls, map, w.writes, w.fill,      \
	                   w.fill_nb, w.par, fill_stride)
	if (fast) LIZEC_LAUNCH_WRITE(true);
	else LIZEC_LAUNCH_WRITE(false);
#undef LIZEC_LAUNCH_WRITE
}

extern "C" int64_t lizec_impl_chunk_write_check(
    int rows, const uint8_t *gftbls, const lizec_chunk_write *writes,
    int num_writes, const uint64_t *fill_ptrs, const uint32_t *fill_nblocks,
    int view_parts, uint32_t fill_block_stride, const uint64_t *par_ptrs,
    uint64_t *bits_out, uint64_t *tiles16_out, uint64_t *tiles8_out,
    uint64_t *ncrc_out);

extern "C" int lizec_chunk_write_batch(
    lizec_engine *e, int rows, const uint8_t *gftbls,
    const lizec_chunk_write *writes, int num_writes,
    const uint64_t *fill_dptrs, const uint32_t *fill_nblocks, int view_parts,
    uint32_t fill_block_stride, const uint64_t *par_dptrs, void *stream) {
	if (!e) return LIZEC_EINVAL;
	uint64_t bits, tiles16, tiles8, ncrc;
	int64_t entries = lizec_impl_chunk_write_check(
	    rows, gftbls, writes, num_writes, fill_dptrs, fill_nblocks, view_parts,
	    fill_block_stride, par_dptrs, &bits, &tiles16, &tiles8, &ncrc);
	if (entries <= 0) return LIZEC_EINVAL;
	const bool fast = (bits & 15) == 0;
	hipStream_t s = stream ? (hipStream_t)stream : e->stream;
	LIZEC_CHECK(hipSetDevice(e->device));

	/* which tile sizes the passes use (ec_chunks_for): a last pass of up to
	 * 4 rows cuts 16 KiB tiles, every other pass 8 KiB ones */
	const int last = rows % 8 ? rows % 8 : 8;
	const bool use16 = last <= 4, use8 = rows > 8 || last > 4;
	/* the ragged call's scratch: table, tile maps, the writes, the fill
	 * counts and the CRC lengths; every section 16-byte aligned.  The u64
	 * scratch holds the fill and parity addresses, the CRC ranges'
	 * addresses and result addresses, and the ranges kernel's results. */
	auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
	const size_t W = (size_t)num_writes, ks = (size_t)view_parts;
	const size_t nfill = W * ks, npar = W * rows;
	size_t ntbl = ks * rows;   /* 32 B each */
	size_t o_map16 = up16(ntbl * kECTblBytes);
	size_t o_map8 = o_map16 + (use16 ? (size_t)tiles16 * 16 : 0);
	size_t o_wr = o_map8 + (use8 ? (size_t)tiles8 * 16 : 0);
	size_t o_fnb = o_wr + up16(W * sizeof(lizec_chunk_write));
	size_t o_len = o_fnb + up16(nfill * 4);
	size_t bytes = o_len + up16((size_t)ncrc * 4);
	/* uploaded slots, and behind them the ranges kernel's results */
	const size_t slots = nfill + npar + 2 * (size_t)ncrc;
	lizec_stream_ctx *c;
	int r = ctx_acquire_ragged(e, s, slots + ((size_t)ncrc + 1) / 2, slots * 8,
	                           bytes, &c);
	if (r != LIZEC_OK) return r;
	uint8_t *h = c->h_ragged;
	for (size_t i = 0; i < ntbl; ++i)
		pack_mixed_radix(gftbls + i * 32, h + i * kECTblBytes);
	memcpy(h + o_wr, writes, W * sizeof(lizec_chunk_write));
	memcpy(h + o_fnb, fill_nblocks, nfill * 4);
	uint64_t *pstage = (uint64_t *)(c->h_staging + (size_t)kECTblBytes * 32 * 32);
	memcpy(pstage, fill_dptrs, nfill * 8);
	memcpy(pstage + nfill, par_dptrs, npar * 8);
	/* one host pass builds the tile maps and the CRC ranges: the new blocks,
	 * then the wanted parities of every touched row */
	uint32_t *m16 = (uint32_t *)(h + o_map16), *m8 = (uint32_t *)(h + o_map8);
	uint32_t *lens = (uint32_t *)(h + o_len);
	uint64_t *addrs = pstage + nfill + npar, *outs = addrs + ncrc;
	size_t nr = 0;
	for (size_t i = 0; i < W; ++i) {
		const lizec_chunk_write &w = writes[i];
		const uint32_t size = w.to - w.from;
		const uint32_t r0 = w.first_block / (uint32_t)ks;
		const uint32_t r1 = (w.first_block + w.block_count - 1) / (uint32_t)ks;
		const uint64_t *pp = par_dptrs + i * rows;
		if (w.crcs)
			for (uint32_t b = 0; b < w.block_count; ++b) {
				addrs[nr] = w.data + (b ? (uint64_t)b * w.data_stride : 0);
				lens[nr] = size;
				outs[nr++] = w.crcs + 4ull * b;
			}
		for (uint32_t b = r0; b <= r1; ++b) {
			if (use16)
				for (uint32_t t = 0; t * 16384u < size; ++t) {
					*m16++ = (uint32_t)i;
					*m16++ = b;
					*m16++ = t;
					*m16++ = b - r0;
				}
			if (use8)
				for (uint32_t t = 0; t * 8192u < size; ++t) {
					*m8++ = (uint32_t)i;
					*m8++ = b;
					*m8++ = t;
					*m8++ = b - r0;
				}
			if (!w.crcs) continue;
			for (int l = 0; l < rows; ++l) {
				if (!pp[l]) continue;
				addrs[nr] =
				    pp[l] + (b > r0 ? (uint64_t)(b - r0) * w.par_stride : 0);
				lens[nr] = size;
				outs[nr++] = w.crcs + 4ull * (w.block_count +
				                              (uint64_t)(b - r0) * rows + l);
			}
		}
	}
	(void)nr;   /* == ncrc: the check function counted the same ranges */
	LIZEC_CHECK(hipMemcpyAsync(c->d_ragged, h, bytes, hipMemcpyHostToDevice, s));
	LIZEC_CHECK(hipMemcpyAsync(c->d_ptrs, pstage, slots * 8,
	                           hipMemcpyHostToDevice, s));
	LIZEC_CHECK(hipEventRecord(c->uploaded, s));
	c->ev_recorded = true;

	write_dev wd;
	wd.tbls = c->d_ragged;
	wd.map16 = (const uint4 *)(c->d_ragged + o_map16);
	wd.map8 = (const uint4 *)(c->d_ragged + o_map8);
	wd.tiles16 = (uint32_t)tiles16;
	wd.tiles8 = (uint32_t)tiles8;
	wd.writes = (const lizec_chunk_write *)(c->d_ragged + o_wr);
	wd.fill_nb = (const uint32_t *)(c->d_ragged + o_fnb);
	wd.fill = c->d_ptrs;
	wd.par = c->d_ptrs + nfill;
	/* passes of at most 8 table rows, as run_batch_strided.  A write none of
	 * whose parities is wanted still has tiles; they return at once. */
	for (int base = 0; base < rows;) {
		int d = rows - base;
		if (d > 8) d = 8;
#define LIZEC_LAUNCH_WRITE_D(D)                                            \
	launch_chunk_write<D>(view_parts, base, rows, wd, fill_block_stride,   \
	                      fast, s)
		switch (d) {
		case 1: LIZEC_LAUNCH_WRITE_D(1); break;
		case 2: LIZEC_LAUNCH_WRITE_D(2); break;
		case 3: LIZEC_LAUNCH_WRITE_D(3); break;
		case 4: LIZEC_LAUNCH_WRITE_D(4); break;
		case 5: LIZEC_LAUNCH_WRITE_D(5); break;
		case 6: LIZEC_LAUNCH_WRITE_D(6); break;
		case 7: LIZEC_LAUNCH_WRITE_D(7); break;
		default: LIZEC_LAUNCH_WRITE_D(8); break;
		}
#undef LIZEC_LAUNCH_WRITE_D
		base += d;
	}
	LIZEC_CHECK(hipGetLastError());
	if (ncrc) {
		/* behind the parity passes on the same stream: the parity ranges are
		 * complete when the ranges kernel starts */
		const uint32_t n = (uint32_t)ncrc;
		uint32_t *d_crcs = (uint32_t *)(c->d_ptrs + nfill + npar + 2 * ncrc);
		r = launch_crc_ranges(e, c->d_ptrs + nfill + npar,
		                      (const uint32_t *)(c->d_ragged + o_len), n, 0u,
		                      d_crcs, nullptr, s);
		if (r != LIZEC_OK) return r;
		hipLaunchKernelGGL(chunk_write_crc_scatter_kernel,
		                   dim3((n + kCrcRangesThreads - 1) / kCrcRangesThreads),
		                   dim3(kCrcRangesThreads), 0, s, d_crcs,
		                   c->d_ptrs + nfill + npar + ncrc, n);
		LIZEC_CHECK(hipGetLastError());
	}
	return LIZEC_OK;
}

/* ------------------------------------------------------------------ */
/* Degraded chunk writes: the same, with lost fill columns rebuilt in  */
/* the parity pass (ec_kernel_write_degraded.h)                        */
/* ------------------------------------------------------------------ */

struct write_degraded_dev {
	const uint8_t *tbls;
	const uint32_t *masks, *index;
	const uint4 *map16, *map8;   /* tile maps for 16 KiB / 8 KiB tiles */
	uint32_t tiles16, tiles8;
	const lizec_chunk_write *writes;
	const uint64_t *old, *par;
	const uint32_t *old_nb;
};

/* One pass of the degraded write kernel, as launch_chunk_write. */
template <int D>
static void launch_chunk_write_degraded(int ks, int srcs, int dest_base,
                                        int rows, const write_degraded_dev &w,
                                        uint32_t old_stride, bool fast,
                                        hipStream_t s) {
	constexpr int CH = ec_chunks_for(D);
	const uint32_t total_tiles = CH == 4 ? w.tiles16 : w.tiles8;
	const uint4 *map = CH == 4 ? w.map16 : w.map8;
	size_t lds = (size_t)D * (ks + srcs) * kECTblBytes;
#define LIZEC_LAUNCH_WRITE_DEG(FAST)                                        \
	hipLaunchKernelGGL(                                                     \
	    HIP_KERNEL_NAME(ec_chunk_write_degraded_kernel<D, CH, FAST>),       \
	    dim3(total_tiles), dim3(kThreads), lds, s, ks, srcs, dest_base,     \
	    rows, w.tbls, w.masks, w.index, map, w.writes, w.old, w.old_nb,     \
	    w.par, old_stride)
	if (fast) LIZEC_LAUNCH_WRITE_DEG(true);
	else LIZEC_LAUNCH_WRITE_DEG(false);
#undef LIZEC_LAUNCH_WRITE_DEG
}

extern "C" int64_t lizec_impl_chunk_write_degraded_check(
    int rows, const uint8_t *gftbls, int ntables, const uint32_t *use_masks,
    const uint32_t *tbl_index, const lizec_chunk_write *writes, int num_writes,
    const uint64_t *old_ptrs, const uint32_t *old_nblocks, int srcs,
    int view_parts, uint32_t old_block_stride, const uint64_t *par_ptrs,
    uint64_t *bits_out, uint64_t *tiles16_out, uint64_t *tiles8_out,
    uint64_t *ncrc_out);

extern "C" int lizec_chunk_write_degraded_batch(
    lizec_engine *e, int rows, const uint8_t *gftbls, int ntables,
    const uint32_t *use_masks, const uint32_t *tbl_index,
    const lizec_chunk_write *writes, int num_writes,
    const uint64_t *old_dptrs, const uint32_t *old_nblocks, int srcs,
    int view_parts, uint32_t old_block_stride, const uint64_t *par_dptrs,
    void *stream) {
	if (!e) return LIZEC_EINVAL;
	uint64_t bits, tiles16, tiles8, ncrc;
	int64_t entries = lizec_impl_chunk_write_degraded_check(
	    rows, gftbls, ntables, use_masks, tbl_index, writes, num_writes,
	    old_dptrs, old_nblocks, srcs, view_parts, old_block_stride, par_dptrs,
	    &bits, &tiles16, &tiles8, &ncrc);
	if (entries <= 0) return LIZEC_EINVAL;
	const bool fast = (bits & 15) == 0;
	hipStream_t s = stream ? (hipStream_t)stream : e->stream;
	LIZEC_CHECK(hipSetDevice(e->device));

	/* lizec_chunk_write_batch's scratch, with the tables' masks and the
	 * writes' table indices behind the tables */
	const int last = rows % 8 ? rows % 8 : 8;
	const bool use16 = last <= 4, use8 = rows > 8 || last > 4;
	auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
	const size_t W = (size_t)num_writes, ks = (size_t)view_parts;
	const size_t nold = W * srcs, npar = W * rows;
	size_t ntbl = (size_t)ntables * rows * (ks + srcs);   /* 32 B each */
	size_t o_mask = up16(ntbl * kECTblBytes);
	size_t o_index = o_mask + up16((size_t)ntables * 4);
	size_t o_map16 = o_index + up16(W * 3 * 4);
	size_t o_map8 = o_map16 + (use16 ? (size_t)tiles16 * 16 : 0);
	size_t o_wr = o_map8 + (use8 ? (size_t)tiles8 * 16 : 0);
	size_t o_onb = o_wr + up16(W * sizeof(lizec_chunk_write));
	size_t o_len = o_onb + up16(nold * 4);
	size_t bytes = o_len + up16((size_t)ncrc * 4);
	const size_t slots = nold + npar + 2 * (size_t)ncrc;
	lizec_stream_ctx *c;
	int r = ctx_acquire_ragged(e, s, slots + ((size_t)ncrc + 1) / 2, slots * 8,
	                           bytes, &c);
	if (r != LIZEC_OK) return r;
	uint8_t *h = c->h_ragged;
	for (size_t i = 0; i < ntbl; ++i)
		pack_mixed_radix(gftbls + i * 32, h + i * kECTblBytes);
	memcpy(h + o_mask, use_masks, (size_t)ntables * 4);
	memcpy(h + o_index, tbl_index, W * 3 * 4);
	memcpy(h + o_wr, writes, W * sizeof(lizec_chunk_write));
	memcpy(h + o_onb, old_nblocks, nold * 4);
	uint64_t *pstage = (uint64_t *)(c->h_staging + (size_t)kECTblBytes * 32 * 32);
	memcpy(pstage, old_dptrs, nold * 8);
	memcpy(pstage + nold, par_dptrs, npar * 8);
	uint32_t *m16 = (uint32_t *)(h + o_map16), *m8 = (uint32_t *)(h + o_map8);
	uint32_t *lens = (uint32_t *)(h + o_len);
	uint64_t *addrs = pstage + nold + npar, *outs = addrs + ncrc;
	size_t nr = 0;
	for (size_t i = 0; i < W; ++i) {
		const lizec_chunk_write &w = writes[i];
		const uint32_t size = w.to - w.from;
		const uint32_t r0 = w.first_block / (uint32_t)ks;
		const uint32_t r1 = (w.first_block + w.block_count - 1) / (uint32_t)ks;
		const uint64_t *pp = par_dptrs + i * rows;
		if (w.crcs)
			for (uint32_t b = 0; b < w.block_count; ++b) {
				addrs[nr] = w.data + (b ? (uint64_t)b * w.data_stride : 0);
				lens[nr] = size;
				outs[nr++] = w.crcs + 4ull * b;
			}
		for (uint32_t b = r0; b <= r1; ++b) {
			if (use16)
				for (uint32_t t = 0; t * 16384u < size; ++t) {
					*m16++ = (uint32_t)i;
					*m16++ = b;
					*m16++ = t;
					*m16++ = b - r0;
				}
			if (use8)
				for (uint32_t t = 0; t * 8192u < size; ++t) {
					*m8++ = (uint32_t)i;
					*m8++ = b;
					*m8++ = t;
					*m8++ = b - r0;
				}
			if (!w.crcs) continue;
			for (int l = 0; l < rows; ++l) {
				if (!pp[l]) continue;
				addrs[nr] =
				    pp[l] + (b > r0 ? (uint64_t)(b - r0) * w.par_stride : 0);
				lens[nr] = size;
				outs[nr++] = w.crcs + 4ull * (w.block_count +
				                              (uint64_t)(b - r0) * rows + l);
			}
		}
	}
	(void)nr;   /* == ncrc: the check function counted the same ranges */
	LIZEC_CHECK(hipMemcpyAsync(c->d_ragged, h, bytes, hipMemcpyHostToDevice, s));
	LIZEC_CHECK(hipMemcpyAsync(c->d_ptrs, pstage, slots * 8,
	                           hipMemcpyHostToDevice, s));
	LIZEC_CHECK(hipEventRecord(c->uploaded, s));
	c->ev_recorded = true;

	write_degraded_dev wd;
	wd.tbls = c->d_ragged;
	wd.masks = (const uint32_t *)(c->d_ragged + o_mask);
	wd.index = (const uint32_t *)(c->d_ragged + o_index);
	wd.map16 = (const uint4 *)(c->d_ragged + o_map16);
	wd.map8 = (const uint4 *)(c->d_ragged + o_map8);
	wd.tiles16 = (uint32_t)tiles16;
	wd.tiles8 = (uint32_t)tiles8;
	wd.writes = (const lizec_chunk_write *)(c->d_ragged + o_wr);
	wd.old_nb = (const uint32_t *)(c->d_ragged + o_onb);
	wd.old = c->d_ptrs;
	wd.par = c->d_ptrs + nold;
	for (int base = 0; base < rows;) {
		int d = rows - base;
		if (d > 8) d = 8;
#define LIZEC_LAUNCH_WRITE_DEG_D(D)                                         \
	launch_chunk_write_degraded<D>(view_parts, srcs, base, rows, wd,        \
	                               old_block_stride, fast, s)
		switch (d) {
		case 1: LIZEC_LAUNCH_WRITE_DEG_D(1); break;
		case 2: LIZEC_LAUNCH_WRITE_DEG_D(2); break;
		case 3: LIZEC_LAUNCH_WRITE_DEG_D(3); break;
		case 4: LIZEC_LAUNCH_WRITE_DEG_D(4); break;
		case 5: LIZEC_LAUNCH_WRITE_DEG_D(5); break;
		case 6: LIZEC_LAUNCH_WRITE_DEG_D(6); break;
		case 7: LIZEC_LAUNCH_WRITE_DEG_D(7); break;
		default: LIZEC_LAUNCH_WRITE_DEG_D(8); break;
		}
#undef LIZEC_LAUNCH_WRITE_DEG_D
		base += d;
	}
	LIZEC_CHECK(hipGetLastError());
	if (ncrc) {
		/* behind the parity passes on the same stream, as in
		 * lizec_chunk_write_batch */
		const uint32_t n = (uint32_t)ncrc;
		uint32_t *d_crcs = (uint32_t *)(c->d_ptrs + nold + npar + 2 * ncrc);
		r = launch_crc_ranges(e, c->d_ptrs + nold + npar,
		                      (const uint32_t *)(c->d_ragged + o_len), n, 0u,
		                      d_crcs, nullptr, s);
		if (r != LIZEC_OK) return r;
		hipLaunchKernelGGL(chunk_write_crc_scatter_kernel,
		                   dim3((n + kCrcRangesThreads - 1) / kCrcRangesThreads),
		                   dim3(kCrcRangesThreads), 0, s, d_crcs,
		                   c->d_ptrs + nold + npar + ncrc, n);
		LIZEC_CHECK(hipGetLastError());
	}
	return LIZEC_OK;
}

/* Upload the per-image tables of a scrub / CRC-fill call into the stream's
 * scratch (u64 slots reused): [dptrs u64 x n][doffs u32 x n][coffs][counts] */
static int upload_image_meta(lizec_engine *e, hipStream_t s,
                             const uint64_t *chunk_dptrs,
                             const uint32_t *data_offs,
                             const uint32_t *crc_offs,
                             const uint32_t *block_counts, int nchunks,
                             uint64_t **d_ptrs, uint32_t **d_doffs,
                             uint32_t **d_coffs, uint32_t **d_counts) {
	size_t words = (size_t)nchunks;               /* dptrs */
	size_t meta = words + (3 * words * 4 + 7) / 8;
	size_t bytes = meta * 8;
	lizec_stream_ctx *c;
	int r = ctx_acquire(e, s, meta + 8, bytes, &c);
	if (r != LIZEC_OK) return r;
	*d_ptrs = c->d_ptrs;
	*d_doffs = (uint32_t *)(c->d_ptrs + nchunks);
	*d_coffs = *d_doffs + nchunks;
	*d_counts = *d_coffs + nchunks;
	uint8_t *st = c->h_staging + (size_t)kECTblBytes * 32 * 32;
	memcpy(st, chunk_dptrs, (size_t)nchunks * 8);
	memcpy(st + (size_t)nchunks * 8, data_offs, (size_t)nchunks * 4);
	memcpy(st + (size_t)nchunks * 12, crc_offs, (size_t)nchunks * 4);
	memcpy(st + (size_t)nchunks * 16, block_counts, (size_t)nchunks * 4);
	LIZEC_CHECK(hipMemcpyAsync(c->d_ptrs, st, (size_t)nchunks * 20,
	                           hipMemcpyHostToDevice, s));
	LIZEC_CHECK(hipEventRecord(c->uploaded, s));
	c->ev_recorded = true;
	return LIZEC_OK;
}

/* Host checks shared by the scrub and the CRC fill, made before anything is
 * allocated or enqueued; on success *max_blocks_out is the largest count. */
static int check_image_args(const uint64_t *chunk_dptrs,
                            const uint32_t *data_offs,
                            const uint32_t *crc_offs,
                            const uint32_t *block_counts, int nchunks,
                            uint32_t block_stride, uint32_t crc_stride,
                            uint32_t *max_blocks_out) {
	if (!chunk_dptrs || !data_offs || !crc_offs || !block_counts ||
	    nchunks < 1)
		return LIZEC_EINVAL;
	/* blocks are read in 32-bit words or wider, and must not overlap */
	if (block_stride < 65536u || (block_stride & 3)) return LIZEC_EINVAL;
	uint32_t max_blocks = 0;
	for (int i = 0; i < nchunks; ++i) {
		if (!chunk_dptrs[i] || ((chunk_dptrs[i] + data_offs[i]) & 3))
			return LIZEC_EINVAL;
		if (block_counts[i] > max_blocks) max_blocks = block_counts[i];
	}
	/* the kernel forms b*stride in 32 bits */
	if (max_blocks == 0 ||
	    (uint64_t)max_blocks * block_stride > 0xFFFFFFFFull ||
	    (uint64_t)max_blocks * crc_stride > 0xFFFFFFFFull)
		return LIZEC_EINVAL;
	*max_blocks_out = max_blocks;
	return LIZEC_OK;
}

extern "C" int lizec_scrub_batch_strided(
    lizec_engine *e, const uint64_t *chunk_dptrs, const uint32_t *data_offs,
    const uint32_t *crc_offs, const uint32_t *block_counts, int nchunks,
    uint32_t block_stride, uint32_t crc_stride, int32_t *dev_status_out,
    void *stream) {
	if (!e || !dev_status_out) return LIZEC_EINVAL;
	uint32_t max_blocks = 0;
	int r = check_image_args(chunk_dptrs, data_offs, crc_offs, block_counts,
	                         nchunks, block_stride, crc_stride, &max_blocks);
	if (r != LIZEC_OK) return r;
	hipStream_t s = stream ? (hipStream_t)stream : e->stream;
	LIZEC_CHECK(hipSetDevice(e->device));
	uint64_t *d_ptrs;
	uint32_t *d_doffs, *d_coffs, *d_counts;
	r = upload_image_meta(e, s, chunk_dptrs, data_offs, crc_offs,
	                      block_counts, nchunks, &d_ptrs, &d_doffs,
	                      &d_coffs, &d_counts);
	if (r != LIZEC_OK) return r;
	/* INT32_MAX sentinel = clean */
	LIZEC_CHECK(hipMemsetD32Async((hipDeviceptr_t)dev_status_out, 0x7FFFFFFF,
	                              nchunks, s));
	uint64_t total = (uint64_t)nchunks * max_blocks;
	uint64_t groups = (total + 3) / 4;
	uint32_t grid = (uint32_t)(groups < 131072 ? groups : 131072);
	hipLaunchKernelGGL(HIP_KERNEL_NAME(scrub_chunks_kernel<false>),
	                   dim3(grid), dim3(kThreads), 0, s,
	                   d_ptrs, d_doffs, d_coffs, d_counts, (uint32_t)nchunks,
	                   max_blocks, block_stride, crc_stride, e->d_crc_const,
	                   dev_status_out);
	LIZEC_CHECK(hipGetLastError());
	return LIZEC_OK;
}

/* Launch the WRITE variant on already-device-resident meta arrays (used by
 * the replication pipeline, which stages meta itself). */
static int image_crc_launch(lizec_engine *e, const uint64_t *d_ptrs,
                            const uint32_t *d_doffs, const uint32_t *d_coffs,
                            const uint32_t *d_counts, int nimages,
                            uint32_t max_blocks, uint32_t block_stride,
                            uint32_t crc_stride, hipStream_t s) {
	uint64_t total = (uint64_t)nimages * max_blocks;
	uint64_t groups = (total + 3) / 4;
	uint32_t grid = (uint32_t)(groups < 131072 ? groups : 131072);
	hipLaunchKernelGGL(HIP_KERNEL_NAME(scrub_chunks_kernel<true>),
	                   dim3(grid), dim3(kThreads), 0, s, d_ptrs, d_doffs,
	                   d_coffs, d_counts, (uint32_t)nimages, max_blocks,
	                   block_stride, crc_stride, e->d_crc_const, nullptr);
	LIZEC_CHECK(hipGetLastError());
	return LIZEC_OK;
}

/* The store counterpart of lizec_scrub_batch_strided: compute every block's
 * CRC and write it big-endian into the image. */
extern "C" int lizec_crc_fill_batch_strided(
    lizec_engine *e, const uint64_t *chunk_dptrs, const uint32_t *data_offs,
    const uint32_t *crc_offs, const uint32_t *block_counts, int nchunks,
    uint32_t block_stride, uint32_t crc_stride, void *stream) {
	if (!e) return LIZEC_EINVAL;
	uint32_t max_blocks = 0;
	int r = check_image_args(chunk_dptrs, data_offs, crc_offs, block_counts,
	                         nchunks, block_stride, crc_stride, &max_blocks);
	if (r != LIZEC_OK) return r;
	hipStream_t s = stream ? (hipStream_t)stream : e->stream;
	LIZEC_CHECK(hipSetDevice(e->device));
	uint64_t *d_ptrs;
	uint32_t *d_doffs, *d_coffs, *d_counts;
	r = upload_image_meta(e, s, chunk_dptrs, data_offs, crc_offs,
	                      block_counts, nchunks, &d_ptrs, &d_doffs,
	                      &d_coffs, &d_counts);
	if (r != LIZEC_OK) return r;
	return image_crc_launch(e, d_ptrs, d_doffs, d_coffs, d_counts, nchunks,
	                        max_blocks, block_stride, crc_stride, s);
}

/* MooseFS layout: 64 KiB blocks after the header, 4-byte CRC array. */
extern "C" int lizec_scrub_batch(lizec_engine *e, const uint64_t *chunk_dptrs,
                                 const uint32_t *data_offs,
                                 const uint32_t *crc_offs,
                                 const uint32_t *block_counts, int nchunks,
                                 int32_t *dev_status_out, void *stream) {
	return lizec_scrub_batch_strided(e, chunk_dptrs, data_offs, crc_offs,
	                                 block_counts, nchunks, 65536u, 4u,
	                                 dev_status_out, stream);
}

/* ------------------------------------------------------------------ */
/* Streaming replication pipeline                  */
/* ------------------------------------------------------------------ */

extern "C" int lizec_host_alloc(void **ptr, uint64_t bytes) {
	*ptr = nullptr;
	LIZEC_CHECK(hipHostMalloc(ptr, bytes));
	return LIZEC_OK;
}

extern "C" void lizec_host_free(void *p) {
	(void)hipHostFree(p);
}

/* One double-buffer slot of the replication pipeline. */
struct repl_slot {
	hipStream_t stream = nullptr;
	hipEvent_t done = nullptr;
	uint8_t *d_in = nullptr;    /* B * ic * part_len           */
	uint8_t *d_img = nullptr;   /* B * oc * img_bytes          */
	uint64_t *d_meta = nullptr; /* ptr tables + image meta     */
	uint8_t *h_stage = nullptr; /* pinned: meta + signatures   */
	bool used = false;
};

static void repl_slot_free(repl_slot &sl) {
	(void)hipFree(sl.d_in);
	(void)hipFree(sl.d_img);
	(void)hipFree(sl.d_meta);
	(void)hipHostFree(sl.h_stage);
	if (sl.done) (void)hipEventDestroy(sl.done);
	if (sl.stream) (void)hipStreamDestroy(sl.stream);
	sl = repl_slot();
}

/* Where an emitted image keeps its blocks and CRCs. */
struct repl_layout {
	uint64_t img_bytes;
	uint32_t header_size;    /* zero-filled, then signed; 0 = no header */
	uint32_t data_off;       /* block 0's data */
	uint32_t crc_off;        /* block 0's CRC */
	uint32_t block_stride;
	uint32_t crc_stride;
};

/* The ChunkReplicator::replicate loop (chunk_replicator.cc:139-196) as a
 * host-to-host streaming pipeline: pull surviving parts from host memory
 * (the reference pulls them from peer sockets), recover the erased parts
 * on-GPU, CRC every recovered 64 KiB block (chunk_replicator.cc:189), and
 * emit complete MooseFS part images (chunk.cc:126-188 geometry: caller's
 * signature bytes at 0, BE CRC array at crc_off, blocks at header_size)
 * into caller host buffers — H2D, compute and D2H double-buffered on two
 * streams.  Use lizec_host_alloc'd (pinned) buffers for real overlap;
 * pageable buffers degrade to synchronous copies but stay correct.
 *
 * host_src:  nchunks*ic host addresses (surviving part bytes, part_len each)
 * gftbls:    32*ic*oc recover tables (lizec_rs_tables)
 * sigs:      nchunks*oc signatures, sig_len bytes each
 * host_dst:  nchunks*oc host addresses (header_size + part_len each)
 * sub_batch: chunks per pipeline stage (0 = auto)
 *
 * This is the body of both entry points, lizec_replicate_run (MooseFS
 * images, as described) and lizec_replicate_run_interleaved; they differ
 * only in `lay`, and have checked e, part_len, ic and oc. */
static int replicate_run_impl(lizec_engine *e, uint64_t part_len, int ic,
                              int oc, const uint8_t *gftbls,
                              const uint64_t *host_src, const uint8_t *sigs,
                              uint32_t sig_len, const repl_layout &lay,
                              const uint64_t *host_dst, int nchunks,
                              int sub_batch) {
	LIZEC_CHECK(hipSetDevice(e->device));

	const uint64_t img_bytes = lay.img_bytes;
	const uint32_t header_size = lay.header_size;
	int B = sub_batch;
	if (B <= 0) {
		/* ~2 GiB of device staging per slot (sub_batch 16 at ec(8,2)
		 * measured ~10% over 12; profiles/ROUND2.md) */
		uint64_t per_chunk = (uint64_t)ic * part_len + oc * img_bytes;
		B = (int)(((uint64_t)1 << 31) / per_chunk);
		if (B < 1) B = 1;
		if (B > 64) B = 64;
	}
	if (B > nchunks) B = nchunks;

	/* per-(stripe,part) device pointer tables + per-image CRC meta:
	 * layout in d_meta/h_stage (8-byte aligned blocks):
	 *   [0)              src ptrs   B*ic u64
	 *   [src_end)        dst ptrs   B*oc u64
	 *   [meta_img)       image ptrs B*oc u64
	 *   [meta_off)       doffs/coffs/counts  3 * B*oc u32  */
	const size_t n_src = (size_t)B * ic, n_dst = (size_t)B * oc;
	const size_t meta_words = n_src + n_dst + n_dst + (3 * n_dst * 4 + 7) / 8;
	const size_t stage_bytes = meta_words * 8 + (size_t)B * oc * sig_len;

	uint8_t *d_tbl = nullptr;
	repl_slot sl[2];
	int rc = LIZEC_OK;
	uint8_t packed[kECTblBytes * 32 * 32];
	for (int i = 0; i < ic * oc; ++i)
		pack_mixed_radix(gftbls + (size_t)i * 32, packed + (size_t)i * kECTblBytes);
	if (hipMalloc(&d_tbl, (size_t)kECTblBytes * ic * oc) != hipSuccess)
		return LIZEC_ENOMEM;
	if (hipMemcpy(d_tbl, packed, (size_t)kECTblBytes * ic * oc,
	              hipMemcpyHostToDevice) != hipSuccess) {
		(void)hipFree(d_tbl);
		return LIZEC_EHIP;
	}
	for (int i = 0; i < 2 && rc == LIZEC_OK; ++i) {
		if (hipStreamCreate(&sl[i].stream) != hipSuccess ||
		    hipEventCreateWithFlags(&sl[i].done, hipEventDisableTiming) !=
		        hipSuccess ||
		    hipMalloc(&sl[i].d_in, (size_t)B * ic * part_len) != hipSuccess ||
		    hipMalloc(&sl[i].d_img, (size_t)B * oc * img_bytes) !=
		        hipSuccess ||
		    hipMalloc(&sl[i].d_meta, meta_words * 8) != hipSuccess ||
		    hipHostMalloc(&sl[i].h_stage, stage_bytes) != hipSuccess)
			rc = LIZEC_ENOMEM;
	}

	for (int c0 = 0; c0 < nchunks && rc == LIZEC_OK; c0 += B) {
		int nb = nchunks - c0 < B ? nchunks - c0 : B;
		repl_slot &s = sl[(c0 / B) & 1];
		hipStream_t st = s.stream;
		if (s.used) {
			if (hipEventSynchronize(s.done) != hipSuccess) {
				rc = LIZEC_EHIP;
				break;
			}
		}
		s.used = true;
		/* stage pointer tables + sigs (host side; slot is idle now) */
		uint64_t *h_src = (uint64_t *)s.h_stage;
		uint64_t *h_dst = h_src + n_src;
		uint64_t *h_img = h_dst + n_dst;
		uint32_t *h_off = (uint32_t *)(h_img + n_dst);
		uint32_t *h_coff = h_off + n_dst;
		uint32_t *h_cnt = h_coff + n_dst;
		uint8_t *h_sig = s.h_stage + meta_words * 8;
		const uint32_t nblocks = (uint32_t)(part_len / 65536);
		for (int i = 0; i < nb; ++i)
			for (int j = 0; j < ic; ++j)
				h_src[i * ic + j] = (uint64_t)(s.d_in +
				                               ((size_t)i * ic + j) * part_len);
		for (int i = 0; i < nb; ++i)
			for (int j = 0; j < oc; ++j) {
				size_t n = (size_t)i * oc + j;
				uint64_t img = (uint64_t)(s.d_img + n * img_bytes);
				h_img[n] = img;
				h_dst[n] = img + lay.data_off;
				h_off[n] = lay.data_off;
				h_coff[n] = lay.crc_off;
				h_cnt[n] = nblocks;
			}
		if (sigs)
			memcpy(h_sig, sigs + (size_t)c0 * oc * sig_len,
			       (size_t)nb * oc * sig_len);
		/* enqueue the stage: H2D parts, header init, recover, CRC, D2H */
		for (int i = 0; i < nb && rc == LIZEC_OK; ++i)
			for (int j = 0; j < ic; ++j)
				if (hipMemcpyAsync(s.d_in + ((size_t)i * ic + j) * part_len,
				                   (const void *)host_src[(size_t)(c0 + i) *
				                                          ic + j],
				                   part_len, hipMemcpyHostToDevice,
				                   st) != hipSuccess)
					rc = LIZEC_EHIP;
		if (rc != LIZEC_OK) break;
		if (hipMemcpyAsync(s.d_meta, s.h_stage, meta_words * 8,
		                   hipMemcpyHostToDevice, st) != hipSuccess) {
			rc = LIZEC_EHIP;
			break;
		}
		for (int n = 0; header_size && n < nb * oc && rc == LIZEC_OK; ++n) {
			uint8_t *img = s.d_img + (size_t)n * img_bytes;
			if (hipMemsetAsync(img, 0, header_size, st) != hipSuccess)
				rc = LIZEC_EHIP;
			else if (sigs && sig_len &&
			         hipMemcpyAsync(img, h_sig + (size_t)n * sig_len, sig_len,
			                        hipMemcpyHostToDevice, st) != hipSuccess)
				rc = LIZEC_EHIP;
		}
		if (rc != LIZEC_OK) break;
		uint64_t *d_src = s.d_meta;
		uint64_t *d_dst = s.d_meta + n_src;
		uint64_t *d_img_ptrs = d_dst + n_dst;
		uint32_t *d_off = (uint32_t *)(d_img_ptrs + n_dst);
		uint32_t *d_coff = d_off + n_dst;
		uint32_t *d_cnt = d_coff + n_dst;
		if (lay.block_stride == kECBlockBytes)
			rc = run_batch(part_len, ic, oc, d_tbl, d_src, d_dst,
			               (uint32_t)nb, st);
		else
			/* staged sources are contiguous and aligned; the images are
			 * packed at n*img_bytes, so their blocks start at every
			 * 4-byte phase */
			rc = run_batch_strided(nblocks, ic, oc, d_tbl, d_src, d_dst,
			                       (uint32_t)nb, kECBlockBytes,
			                       lay.block_stride, true, false, st);
		if (rc != LIZEC_OK) break;
		rc = image_crc_launch(e, d_img_ptrs, d_off, d_coff, d_cnt, nb * oc,
		                      nblocks, lay.block_stride, lay.crc_stride, st);
		if (rc != LIZEC_OK) break;
		for (int n = 0; n < nb * oc && rc == LIZEC_OK; ++n)
			if (hipMemcpyAsync((void *)host_dst[(size_t)c0 * oc + n],
			                   s.d_img + (size_t)n * img_bytes, img_bytes,
			                   hipMemcpyDeviceToHost, st) != hipSuccess)
				rc = LIZEC_EHIP;
		if (rc != LIZEC_OK) break;
		if (hipEventRecord(s.done, st) != hipSuccess) rc = LIZEC_EHIP;
	}
	for (int i = 0; i < 2; ++i) {
		if (sl[i].used && sl[i].stream)
			(void)hipStreamSynchronize(sl[i].stream);
		repl_slot_free(sl[i]);
	}
	(void)hipFree(d_tbl);
	return rc;
}

static int check_replicate_args(lizec_engine *e, uint64_t part_len, int ic,
                                int oc, const uint8_t *gftbls,
                                const uint64_t *host_src,
                                const uint64_t *host_dst, int nchunks) {
	if (!e || !gftbls || !host_src || !host_dst || nchunks < 1)
		return LIZEC_EINVAL;
	if (ic < 1 || ic > 32 || oc < 1 || oc > 32) return LIZEC_EINVAL;
	if (part_len == 0 || part_len % 65536 || part_len > (uint64_t)1 << 31)
		return LIZEC_EINVAL;
	return LIZEC_OK;
}

extern "C" int lizec_replicate_run(lizec_engine *e, uint64_t part_len,
                                   int ic, int oc, const uint8_t *gftbls,
                                   const uint64_t *host_src,
                                   const uint8_t *sigs, uint32_t sig_len,
                                   uint32_t header_size, uint32_t crc_off,
                                   const uint64_t *host_dst, int nchunks,
                                   int sub_batch) {
	int r = check_replicate_args(e, part_len, ic, oc, gftbls, host_src,
	                             host_dst, nchunks);
	if (r != LIZEC_OK) return r;
	if (sig_len > header_size || crc_off + 4 * (part_len / 65536) > header_size)
		return LIZEC_EINVAL;
	/* the staged images are packed at n*(header_size + part_len) and their
	 * blocks start header_size in: run_batch reads and writes them with
	 * 16-byte vector accesses and checks no alignment of its own
	 * (check_part_addrs is the public call's) */
	if (header_size % 16) return LIZEC_EINVAL;
	const repl_layout lay = {header_size + part_len, header_size, header_size,
	                         crc_off, kECBlockBytes, 4u};
	return replicate_run_impl(e, part_len, ic, oc, gftbls, host_src, sigs,
	                          sig_len, lay, host_dst, nchunks, sub_batch);
}

/* The same pipeline emitting INTERLEAVED-format images (chunk.cc:191-209):
 * no header and no signature; block b's big-endian CRC at 65540*b, its data
 * right behind it. */
extern "C" int lizec_replicate_run_interleaved(
    lizec_engine *e, uint64_t part_len, int ic, int oc, const uint8_t *gftbls,
    const uint64_t *host_src, const uint64_t *host_dst, int nchunks,
    int sub_batch) {
	int r = check_replicate_args(e, part_len, ic, oc, gftbls, host_src,
	                             host_dst, nchunks);
	if (r != LIZEC_OK) return r;
	constexpr uint32_t kHddBlock = kECBlockBytes + 4;   /* chunk.h:40 */
	const repl_layout lay = {part_len / kECBlockBytes * kHddBlock, 0u, 4u, 0u,
	                         kHddBlock, kHddBlock};
	return replicate_run_impl(e, part_len, ic, oc, gftbls, host_src, nullptr,
	                          0u, lay, host_dst, nchunks, sub_batch);
}

/* ------------------------------------------------------------------ */
/* Ragged streaming rebuild (replicate_stage.h)                       */
/* ------------------------------------------------------------------ */

extern "C" int lizec_impl_replicate_ragged_check(
    int ic, int oc, const uint8_t *gftbls, int ntables,
    const uint32_t *tbl_index, const uint64_t *host_src,
    const uint32_t *src_nblocks, const uint64_t *host_src_crc,
    const uint8_t *sigs, uint32_t sig_len, uint32_t header_size,
    uint32_t crc_off, const uint64_t *host_dst, const uint32_t *dst_nblocks,
    int nchunks, uint64_t stage_bytes, uint32_t flags,
    const uint32_t *bad_out);

/* One double-buffer slot of the ragged pipeline.  Everything a stage's
 * kernels read besides the tables lives here — nothing goes through the
 * engine's per-stream scratch, so nothing is left behind under the handle
 * of a stream that dies with the call. */
struct repl_ragged_slot {
	hipStream_t stream = nullptr;
	hipEvent_t done = nullptr;
	uint8_t *d_arena = nullptr;   /* sources, then images, 16-aligned each */
	uint8_t *d_meta = nullptr;    /* repl_stage_meta */
	uint8_t *h_meta = nullptr;    /* pinned mirror */
	bool used = false;
};

static void repl_ragged_slot_free(repl_ragged_slot &sl) {
	(void)hipFree(sl.d_arena);
	(void)hipFree(sl.d_meta);
	(void)hipHostFree(sl.h_meta);
	if (sl.done) (void)hipEventDestroy(sl.done);
	if (sl.stream) (void)hipStreamDestroy(sl.stream);
	sl = repl_ragged_slot();
}

/* A stage's metadata block: byte offsets of its sections, each 16-aligned.
 * One pinned block, one H2D per stage. */
struct repl_stage_meta {
	size_t index;   /* u32 [n]: table of every chunk */
	size_t dmap;    /* uint2 [rows]: block rows of the destinations */
	size_t smap;    /* uint2 [srows]: block rows of the sources (verify) */
	size_t snb;     /* u32 [n][ic] */
	size_t dnb;     /* u32 [n][oc] */
	size_t src;     /* u64 [n][ic]: staged sources */
	size_t dst;     /* u64 [n][oc]: block 0 of every image */
	size_t img;     /* u64 [n][oc]: images, 0 = not wanted */
	size_t doff;    /* u32 [n][oc] x 3: data offset, CRC offset, count */
	size_t crcp;    /* u64 [n][ic]: staged CRC bytes, 0 = not verified */
	size_t bad;     /* u32 [n]: the masks, uploaded as zeros */
	size_t sig;     /* u8 [n][oc][sig_len] */
	size_t crc;     /* u8: the sources' CRC bytes, back to back */
	size_t bytes;
};

static repl_stage_meta repl_stage_layout(size_t n, int ic, int oc,
                                         size_t rows, size_t srows,
                                         size_t sig_bytes, size_t crc_bytes) {
	auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
	repl_stage_meta m;
	m.index = 0;
	m.dmap = m.index + up16(n * 4);
	m.smap = m.dmap + up16(rows * 8);
	m.snb = m.smap + up16(srows * 8);
	m.dnb = m.snb + up16(n * ic * 4);
	m.src = m.dnb + up16(n * oc * 4);
	m.dst = m.src + up16(n * ic * 8);
	m.img = m.dst + up16(n * oc * 8);
	m.doff = m.img + up16(n * oc * 8);
	m.crcp = m.doff + up16(n * oc * 12);
	m.bad = m.crcp + up16(n * ic * 8);
	m.sig = m.bad + up16(n * 4);
	m.crc = m.sig + up16(sig_bytes);
	m.bytes = m.crc + up16(crc_bytes);
	return m;
}

/* What one stage needs: counted once to size the slots, and again when the
 * stage is laid out. */
struct repl_stage_need {
	uint64_t arena;        /* sources + wanted images, 16-rounded each */
	int64_t rows, srows;   /* block rows of destinations / of sources */
	size_t crc_bytes;
	uint32_t max_dst;
};

extern "C" int lizec_replicate_run_ragged(
    lizec_engine *e, int ic, int oc, const uint8_t *gftbls, int ntables,
    const uint32_t *tbl_index, const uint64_t *host_src,
    const uint32_t *src_nblocks, const uint64_t *host_src_crc,
    const uint8_t *sigs, uint32_t sig_len, uint32_t header_size,
    uint32_t crc_off, const uint64_t *host_dst, const uint32_t *dst_nblocks,
    int nchunks, uint64_t stage_bytes, uint32_t flags, uint32_t *bad_out) {
	if (!e) return LIZEC_EINVAL;
	int rc = lizec_impl_replicate_ragged_check(
	    ic, oc, gftbls, ntables, tbl_index, host_src, src_nblocks,
	    host_src_crc, sigs, sig_len, header_size, crc_off, host_dst,
	    dst_nblocks, nchunks, stage_bytes, flags, bad_out);
	if (rc != LIZEC_OK) return rc;
	const bool il = (flags & LIZEC_REPL_INTERLEAVED) != 0;
	constexpr uint32_t kHddBlock = kECBlockBytes + 4;   /* chunk.h:40 */
	const uint32_t hdr = il ? 0u : header_size;
	const uint32_t data_off = il ? 4u : header_size;
	const uint32_t coff = il ? 0u : crc_off;
	const uint32_t bstride = il ? kHddBlock : kECBlockBytes;
	const uint32_t cstride = il ? kHddBlock : 4u;
	const size_t sigl = il || !sigs ? 0 : sig_len;
	auto image_bytes = [&](size_t slot) -> uint64_t {
		if (!host_dst[slot]) return 0;
		return hdr + (uint64_t)dst_nblocks[slot] * bstride;
	};

	int64_t nst = lizec_replicate_ragged_stages(
	    ic, oc, src_nblocks, host_dst, dst_nblocks, nchunks, header_size,
	    flags, stage_bytes, nullptr, 0);
	if (nst < 1) return LIZEC_EINVAL;
	uint32_t *first = (uint32_t *)malloc(((size_t)nst + 1) * 4);
	if (!first) return LIZEC_ENOMEM;
	if (lizec_replicate_ragged_stages(ic, oc, src_nblocks, host_dst,
	                                  dst_nblocks, nchunks, header_size, flags,
	                                  stage_bytes, first,
	                                  (uint64_t)nst + 1) != nst) {
		free(first);
		return LIZEC_EINVAL;
	}
	auto need_of = [&](int64_t i) {
		const uint32_t c0 = first[i], n = first[i + 1] - c0;
		repl_stage_need nd = {0, 0, 0, 0, 0};
		for (size_t s = (size_t)c0 * ic; s < (size_t)(c0 + n) * ic; ++s) {
			nd.arena += (uint64_t)src_nblocks[s] * kECBlockBytes;
			if (host_src_crc && host_src_crc[s])
				nd.crc_bytes += (size_t)src_nblocks[s] * 4;
		}
		for (size_t s = (size_t)c0 * oc; s < (size_t)(c0 + n) * oc; ++s) {
			nd.arena += (image_bytes(s) + 15) & ~(uint64_t)15;
			if (dst_nblocks[s] > nd.max_dst) nd.max_dst = dst_nblocks[s];
		}
		nd.rows = lizec_ragged_block_map(dst_nblocks + (size_t)c0 * oc, oc,
		                                 (int)n, nullptr, 0);
		if (host_src_crc)
			nd.srows = lizec_ragged_block_map(src_nblocks + (size_t)c0 * ic,
			                                  ic, (int)n, nullptr, 0);
		return nd;
	};
	/* the slots are sized for the largest stage */
	uint64_t arena_max = 16;
	size_t meta_max = 0;
	for (int64_t i = 0; i < nst; ++i) {
		const repl_stage_need nd = need_of(i);
		if (nd.rows < 0 || nd.srows < 0) {
			free(first);
			return LIZEC_EINVAL;
		}
		const size_t n = first[i + 1] - first[i];
		const size_t mb = repl_stage_layout(n, ic, oc, (size_t)nd.rows,
		                                    (size_t)nd.srows, n * oc * sigl,
		                                    nd.crc_bytes).bytes;
		if (nd.arena > arena_max) arena_max = nd.arena;
		if (mb > meta_max) meta_max = mb;
	}
	if (bad_out && !host_src_crc) memset(bad_out, 0, (size_t)nchunks * 4);

	if (hipSetDevice(e->device) != hipSuccess) {
		free(first);
		return LIZEC_EHIP;
	}
	const size_t tbl_bytes = (size_t)kECTblBytes * ntables * ic * oc;
	uint8_t *d_tbl = nullptr, *h_tbl = (uint8_t *)malloc(tbl_bytes);
	repl_ragged_slot sl[2];
	if (!h_tbl) rc = LIZEC_ENOMEM;
	if (rc == LIZEC_OK) {
		for (size_t i = 0; i < (size_t)ntables * ic * oc; ++i)
			pack_mixed_radix(gftbls + i * 32, h_tbl + i * kECTblBytes);
		if (hipMalloc(&d_tbl, tbl_bytes) != hipSuccess)
			rc = LIZEC_ENOMEM;
		else if (hipMemcpy(d_tbl, h_tbl, tbl_bytes, hipMemcpyHostToDevice) !=
		         hipSuccess)
			rc = LIZEC_EHIP;
	}
	for (int i = 0; i < 2 && i < nst && rc == LIZEC_OK; ++i) {
		if (hipStreamCreate(&sl[i].stream) != hipSuccess ||
		    hipEventCreateWithFlags(&sl[i].done, hipEventDisableTiming) !=
		        hipSuccess ||
		    hipMalloc(&sl[i].d_arena, arena_max) != hipSuccess ||
		    hipMalloc(&sl[i].d_meta, meta_max) != hipSuccess ||
		    hipHostMalloc(&sl[i].h_meta, meta_max) != hipSuccess)
			rc = LIZEC_ENOMEM;
	}

	for (int64_t i = 0; i < nst && rc == LIZEC_OK; ++i) {
		const uint32_t c0 = first[i], n = first[i + 1] - c0;
		const repl_stage_need nd = need_of(i);
		const repl_stage_meta m =
		    repl_stage_layout(n, ic, oc, (size_t)nd.rows, (size_t)nd.srows,
		                      (size_t)n * oc * sigl, nd.crc_bytes);
		repl_ragged_slot &s = sl[i & 1];
		hipStream_t st = s.stream;
		if (s.used && hipEventSynchronize(s.done) != hipSuccess) {
			rc = LIZEC_EHIP;
			break;
		}
		s.used = true;
		/* lay the stage out (host side; the slot is idle now) */
		uint8_t *h = s.h_meta;
		const size_t nsrc = (size_t)n * ic, ndst = (size_t)n * oc;
		const uint64_t *hs = host_src + (size_t)c0 * ic;
		const uint64_t *hd = host_dst + (size_t)c0 * oc;
		const uint32_t *sn = src_nblocks + (size_t)c0 * ic;
		const uint32_t *dn = dst_nblocks + (size_t)c0 * oc;
		if (tbl_index)
			memcpy(h + m.index, tbl_index + c0, (size_t)n * 4);
		else
			memset(h + m.index, 0, (size_t)n * 4);
		if ((nd.rows &&
		     lizec_ragged_block_map(dn, oc, (int)n, (uint32_t *)(h + m.dmap),
		                            (uint64_t)nd.rows) != nd.rows) ||
		    (nd.srows &&
		     lizec_ragged_block_map(sn, ic, (int)n, (uint32_t *)(h + m.smap),
		                            (uint64_t)nd.srows) != nd.srows)) {
			rc = LIZEC_EINVAL;
			break;
		}
		memcpy(h + m.snb, sn, nsrc * 4);
		memcpy(h + m.dnb, dn, ndst * 4);
		uint64_t *h_src = (uint64_t *)(h + m.src);
		uint64_t *h_dst = (uint64_t *)(h + m.dst);
		uint64_t *h_img = (uint64_t *)(h + m.img);
		uint32_t *h_doff = (uint32_t *)(h + m.doff);
		uint32_t *h_coff = h_doff + ndst, *h_cnt = h_coff + ndst;
		uint64_t *h_crcp = (uint64_t *)(h + m.crcp);
		uint64_t off = 0;
		size_t crc_at = m.crc;
		for (size_t k = 0; k < nsrc; ++k) {
			h_src[k] = sn[k] ? (uint64_t)(s.d_arena + off) : 0;
			off += (uint64_t)sn[k] * kECBlockBytes;
			h_crcp[k] = 0;
			const uint64_t crcs = host_src_crc ? host_src_crc[(size_t)c0 * ic + k] : 0;
			if (crcs) {
				/* the CRC bytes travel with the metadata; a slot of no
				 * blocks keeps an address, which is never read */
				h_crcp[k] = (uint64_t)(s.d_meta + crc_at);
				memcpy(h + crc_at, (const void *)crcs, (size_t)sn[k] * 4);
				crc_at += (size_t)sn[k] * 4;
			}
		}
		const uint64_t img0 = off;
		for (size_t k = 0; k < ndst; ++k) {
			const uint64_t bytes = image_bytes((size_t)c0 * oc + k);
			h_img[k] = hd[k] ? (uint64_t)(s.d_arena + off) : 0;
			h_dst[k] = dn[k] ? h_img[k] + data_off : 0;
			h_doff[k] = data_off;
			h_coff[k] = coff;
			h_cnt[k] = dn[k];
			off += (bytes + 15) & ~(uint64_t)15;
		}
		memset(h + m.bad, 0, (size_t)n * 4);
		if (sigl)
			memcpy(h + m.sig, sigs + (size_t)c0 * oc * sigl, ndst * sigl);
		/* enqueue the stage: H2D parts and metadata, headers, verify,
		 * recover, CRC, D2H */
		off = 0;
		for (size_t k = 0; k < nsrc && rc == LIZEC_OK; ++k) {
			const uint64_t bytes = (uint64_t)sn[k] * kECBlockBytes;
			if (bytes &&
			    hipMemcpyAsync(s.d_arena + off, (const void *)hs[k], bytes,
			                   hipMemcpyHostToDevice, st) != hipSuccess)
				rc = LIZEC_EHIP;
			off += bytes;
		}
		if (rc != LIZEC_OK) break;
		if (hipMemcpyAsync(s.d_meta, h, m.bytes, hipMemcpyHostToDevice, st) !=
		    hipSuccess) {
			rc = LIZEC_EHIP;
			break;
		}
		uint8_t *d = s.d_meta;
		if (hdr)
			hipLaunchKernelGGL(replicate_header_kernel, dim3((uint32_t)ndst),
			                   dim3(kReplHeaderThreads), 0, st,
			                   (const uint64_t *)(d + m.img), d + m.sig,
			                   (uint32_t)sigl, hdr);
		if (nd.srows) {
			/* one wave per (source block row, slot), four per workgroup */
			const uint64_t items = (uint64_t)nd.srows * ic;
			hipLaunchKernelGGL(replicate_verify_kernel,
			                   dim3((uint32_t)((items + 3) / 4)),
			                   dim3(kCrcRangesThreads), 0, st, ic, items,
			                   (const uint2 *)(d + m.smap),
			                   (const uint64_t *)(d + m.src),
			                   (const uint64_t *)(d + m.crcp),
			                   (const uint32_t *)(d + m.snb), e->d_crc_const,
			                   e->d_crc_const + kCrcTabWords,
			                   (uint32_t *)(d + m.bad));
		}
		if (nd.rows) {
			/* a stage without a block reaches neither launch: both refuse
			 * an empty batch */
			ragged_dev rd;
			rd.tbls = d_tbl;
			rd.index = (const uint32_t *)(d + m.index);
			rd.map = (const uint2 *)(d + m.dmap);
			rd.src = (const uint64_t *)(d + m.src);
			rd.dst = (const uint64_t *)(d + m.dst);
			rd.src_nb = (const uint32_t *)(d + m.snb);
			rd.dst_nb = (const uint32_t *)(d + m.dnb);
			/* staged sources are 16-aligned; MooseFS blocks too, INTERLEAVED
			 * ones sit at 4 + 65540*b and take the 4-byte path */
			launch_ec_ragged_passes((uint32_t)nd.rows, ic, oc, rd,
			                        kECBlockBytes, bstride, true, !il, st);
			if (hipGetLastError() != hipSuccess) {
				rc = LIZEC_EHIP;
				break;
			}
			rc = image_crc_launch(e, (const uint64_t *)(d + m.img),
			                      (const uint32_t *)(d + m.doff),
			                      (const uint32_t *)(d + m.doff) + ndst,
			                      (const uint32_t *)(d + m.doff) + 2 * ndst,
			                      (int)ndst, nd.max_dst, bstride, cstride, st);
			if (rc != LIZEC_OK) break;
		}
		if (hipGetLastError() != hipSuccess) {
			rc = LIZEC_EHIP;
			break;
		}
		off = img0;
		for (size_t k = 0; k < ndst && rc == LIZEC_OK; ++k) {
			const uint64_t bytes = image_bytes((size_t)c0 * oc + k);
			if (bytes &&
			    hipMemcpyAsync((void *)hd[k], s.d_arena + off, bytes,
			                   hipMemcpyDeviceToHost, st) != hipSuccess)
				rc = LIZEC_EHIP;
			off += (bytes + 15) & ~(uint64_t)15;
		}
		if (rc != LIZEC_OK) break;
		if (host_src_crc &&
		    hipMemcpyAsync(bad_out + c0, d + m.bad, (size_t)n * 4,
		                   hipMemcpyDeviceToHost, st) != hipSuccess) {
			rc = LIZEC_EHIP;
			break;
		}
		if (hipEventRecord(s.done, st) != hipSuccess) rc = LIZEC_EHIP;
	}
	for (int i = 0; i < 2; ++i) {
		if (sl[i].used && sl[i].stream &&
		    hipStreamSynchronize(sl[i].stream) != hipSuccess &&
		    rc == LIZEC_OK)
			rc = LIZEC_EHIP;
		repl_ragged_slot_free(sl[i]);
	}
	(void)hipFree(d_tbl);
	free(h_tbl);
	free(first);
	return rc;
}
