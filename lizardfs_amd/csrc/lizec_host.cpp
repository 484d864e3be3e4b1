/* lizec_host.cpp — host side of the MI355X EC engine: GF(2^8) matrix
 * algebra, ISA-L-shaped drop-in surface, CRC32, slice-type algebra.
 *
 * Semantics follow the reference (lizardfs/lizardfs) interfaces cited in
 * include/lizec.h; the implementation is our own (carry-less polynomial
 * multiply + Fermat inverse instead of log/exp tables, slicing-by-8 CRC).
 * Bit-exactness vs the reference is enforced by tests/ against the oracle
 * and the committed golden vectors.
 */
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/lizec.h"

/* ------------------------------------------------------------------ */
/* GF(2^8), polynomial 0x11D                                          */
/* ------------------------------------------------------------------ */

namespace {

/* Carry-less 8x8 multiply, then reduce mod x^8+x^4+x^3+x^2+1. */
inline uint8_t gfmul(uint8_t a, uint8_t b) {
	uint32_t r = 0;
	uint32_t aa = a;
	for (int i = 0; i < 8; ++i)
		if ((b >> i) & 1) r ^= aa << i;
	/* reduce bits 15..8 */
	for (int i = 15; i >= 8; --i)
		if ((r >> i) & 1) r ^= 0x11Du << (i - 8);
	return (uint8_t)r;
}

inline uint8_t gfinv(uint8_t a) {
	if (a == 0) return 0;
	/* a^254 = a^-1 in GF(256): square-and-multiply. */
	uint8_t r = 1, p = a;
	int e = 254;
	while (e) {
		if (e & 1) r = gfmul(r, p);
		p = gfmul(p, p);
		e >>= 1;
	}
	return r;
}

}  // namespace

extern "C" void gf_gen_rs_matrix(uint8_t *a, int m, int k) {
	memset(a, 0, (size_t)k * m);
	for (int i = 0; i < k; ++i) a[k * i + i] = 1;
	uint8_t gen = 1;
	for (int i = k; i < m; ++i) {
		uint8_t p = 1;
		for (int j = 0; j < k; ++j) {
			a[k * i + j] = p;
			p = gfmul(p, gen);
		}
		gen = gfmul(gen, 2);
	}
}

extern "C" void gf_gen_cauchy1_matrix(uint8_t *a, int m, int k) {
	memset(a, 0, (size_t)k * m);
	for (int i = 0; i < k; ++i) a[k * i + i] = 1;
	uint8_t *p = &a[k * k];
	for (int i = k; i < m; ++i)
		for (int j = 0; j < k; ++j)
			*p++ = gfinv((uint8_t)(i ^ j));
}

extern "C" int gf_invert_matrix(uint8_t *in_mat, uint8_t *out_mat, const int n) {
	for (int i = 0; i < n * n; ++i) out_mat[i] = 0;
	for (int i = 0; i < n; ++i) out_mat[i * n + i] = 1;

	for (int i = 0; i < n; ++i) {
		if (in_mat[i * n + i] == 0) {
			int j = i + 1;
			for (; j < n; ++j)
				if (in_mat[j * n + i]) break;
			if (j == n) return -1;
			for (int c = 0; c < n; ++c) {
				uint8_t t = in_mat[i * n + c];
				in_mat[i * n + c] = in_mat[j * n + c];
				in_mat[j * n + c] = t;
				t = out_mat[i * n + c];
				out_mat[i * n + c] = out_mat[j * n + c];
				out_mat[j * n + c] = t;
			}
		}
		uint8_t piv = gfinv(in_mat[i * n + i]);
		for (int c = 0; c < n; ++c) {
			in_mat[i * n + c] = gfmul(in_mat[i * n + c], piv);
			out_mat[i * n + c] = gfmul(out_mat[i * n + c], piv);
		}
		for (int r = 0; r < n; ++r) {
			if (r == i) continue;
			uint8_t f = in_mat[r * n + i];
			if (!f) continue;
			for (int c = 0; c < n; ++c) {
				in_mat[r * n + c] ^= gfmul(f, in_mat[i * n + c]);
				out_mat[r * n + c] ^= gfmul(f, out_mat[i * n + c]);
			}
		}
	}
	return 0;
}

extern "C" void ec_init_tables(int k, int rows, uint8_t *a, uint8_t *g_tbls) {
	int n = k * rows;   /* linear expansion; layout [row][col][32] */
	for (int i = 0; i < n; ++i) {
		uint8_t c = a[i];
		uint8_t *t = g_tbls + (size_t)i * 32;
		for (int v = 0; v < 16; ++v) {
			t[v] = gfmul(c, (uint8_t)v);
			t[16 + v] = gfmul(c, (uint8_t)(v << 4));
		}
	}
}

extern "C" void ec_encode_data(int len, int srcs, int dests, uint8_t *v,
                               uint8_t **src, uint8_t **dest) {
	for (int l = 0; l < dests; ++l) {
		uint8_t *vl = v + (size_t)l * srcs * 32;
		uint8_t *d = dest[l];
		for (int i = 0; i < len; ++i) {
			uint8_t s = 0;
			const uint8_t *tbl = vl;
			for (int j = 0; j < srcs; ++j) {
				uint8_t a = src[j][i];
				s ^= tbl[a & 0xF] ^ tbl[16 + (a >> 4)];
				tbl += 32;
			}
			d[i] = s;
		}
	}
}


/* distinct-name C entry points for the C++-mangled alias TU
 * (lizec_abi_aliases.cpp) — avoids linkage conflicts in one TU. */
extern "C" void lizec_impl_gen_rs_matrix(uint8_t *a, int m, int k) {
	gf_gen_rs_matrix(a, m, k);
}
extern "C" void lizec_impl_gen_cauchy1_matrix(uint8_t *a, int m, int k) {
	gf_gen_cauchy1_matrix(a, m, k);
}
extern "C" int lizec_impl_invert_matrix(uint8_t *in_mat, uint8_t *out_mat,
                                        int n) {
	return gf_invert_matrix(in_mat, out_mat, n);
}
extern "C" void lizec_impl_init_tables(int k, int rows, uint8_t *a,
                                       uint8_t *g_tbls) {
	ec_init_tables(k, rows, a, g_tbls);
}
extern "C" void lizec_impl_encode_data(int len, int srcs, int dests,
                                       uint8_t *v, uint8_t **src,
                                       uint8_t **dest) {
	ec_encode_data(len, srcs, dests, v, src, dest);
}

/* ------------------------------------------------------------------ */
/* ReedSolomon table builders (reed_solomon.h:41-373 semantics)       */
/* ------------------------------------------------------------------ */

namespace {

constexpr int MAXK = 32, MAXM = 32, MAXP = 64;

inline int popcount(uint64_t x) { return __builtin_popcountll(x); }

void select_rows(uint8_t *out, const uint8_t *in, int s1, int s2,
                 uint64_t rows) {
	for (int i = 0; i < s1; ++i, in += s2)
		if ((rows >> i) & 1) {
			memcpy(out, in, (size_t)s2);
			out += s2;
		}
}

void select_columns(uint8_t *out, const uint8_t *in, int s1, int s2,
                    uint64_t cols) {
	for (int i = 0; i < s1; ++i, in += s2)
		for (int j = 0; j < s2; ++j)
			if ((cols >> j) & 1) *out++ = in[j];
}

}  // namespace

extern "C" int lizec_rs_tables(int k, int m, uint64_t present_mask,
                               uint64_t nonnull_mask, uint64_t needed_mask,
                               uint8_t *gftbls, int *in_count, int *out_count) {
	if (k < 1 || k > MAXK || m < 1 || m > MAXM) return LIZEC_EINVAL;
	int nparts = k + m;
	uint64_t all = (nparts == 64) ? ~0ULL : (((uint64_t)1 << nparts) - 1);
	present_mask &= all;
	nonnull_mask &= present_mask;
	needed_mask &= all & ~present_mask;
	if (popcount(~present_mask & all) != m) return LIZEC_EINVAL;

	uint8_t rs_matrix[MAXP * MAXK];
	if (m >= 5 || (m == 4 && k > 20))
		gf_gen_cauchy1_matrix(rs_matrix, nparts, k);
	else
		gf_gen_rs_matrix(rs_matrix, nparts, k);

	/* non_zero_input indexed by surviving-part ORDER (reed_solomon.h:103-108) */
	uint64_t non_zero_input = 0;
	int in_with_zero = 0, data_present = 0;
	for (int i = 0; i < nparts; ++i) {
		if ((present_mask >> i) & 1) {
			if ((nonnull_mask >> i) & 1)
				non_zero_input |= (uint64_t)1 << in_with_zero;
			in_with_zero++;
			data_present += (i < k);
		}
	}
	int nz = popcount(non_zero_input);
	int needed_count = popcount(needed_mask);
	int parity_needed = popcount(needed_mask >> k);
	if (needed_count == 0 || nz == 0) return LIZEC_EINVAL;

	uint8_t work[MAXP * MAXK];
	uint8_t recover_m[MAXP * MAXK];

	if (data_present == k) {
		/* createEncodingMatrix (reed_solomon.h:189-217) */
		select_rows(recover_m, rs_matrix, nparts, k, needed_mask);
	} else {
		/* createRecoveryMatrix (reed_solomon.h:229-281) */
		uint8_t decode_m[MAXK * MAXK];
		select_rows(work, rs_matrix, nparts, k, present_mask);
		if (gf_invert_matrix(work, decode_m, k) != 0) return LIZEC_ESINGULAR;
		if (parity_needed > 0) {
			uint8_t sel[MAXP * MAXK];
			select_rows(sel, rs_matrix, nparts, k, needed_mask);
			/* recover = sel x decode  (matrixMultiply, reed_solomon.h:344) */
			for (int i = 0; i < needed_count; ++i)
				for (int c = 0; c < k; ++c) {
					uint8_t s = 0;
					for (int j = 0; j < k; ++j)
						s ^= gfmul(sel[i * k + j], decode_m[j * k + c]);
					recover_m[i * k + c] = s;
				}
		} else {
			select_rows(recover_m, decode_m, k, k, needed_mask);
		}
	}

	if (nz < k) {
		select_columns(work, recover_m, needed_count, k, non_zero_input);
		ec_init_tables(needed_count, nz, work, gftbls);
	} else {
		ec_init_tables(needed_count, k, recover_m, gftbls);
	}
	if (in_count) *in_count = nz;
	if (out_count) *out_count = needed_count;
	return LIZEC_OK;
}

extern "C" int lizec_rs_encode_tables(int k, int m, uint8_t *gftbls) {
	int ic, oc;
	uint64_t data = ((uint64_t)1 << k) - 1;
	uint64_t par = (((uint64_t)1 << m) - 1) << k;
	return lizec_rs_tables(k, m, data, data, par, gftbls, &ic, &oc);
}

/* ------------------------------------------------------------------ */
/* CRC32 (reflected, poly 0xEDB88320; crc.h:25-31 semantics)          */
/* ------------------------------------------------------------------ */

static uint32_t crc8tab[8][256];
static bool crc_ready = false;

extern "C" void lizec_crc32_init(void) {
	if (crc_ready) return;
	for (uint32_t i = 0; i < 256; ++i) {
		uint32_t c = i;
		for (int b = 0; b < 8; ++b)
			c = (c & 1) ? (0xEDB88320u ^ (c >> 1)) : (c >> 1);
		crc8tab[0][i] = c;
	}
	for (uint32_t i = 0; i < 256; ++i)
		for (int t = 1; t < 8; ++t)
			crc8tab[t][i] = crc8tab[0][crc8tab[t - 1][i] & 0xff] ^
			                (crc8tab[t - 1][i] >> 8);
	crc_ready = true;
}

extern "C" uint32_t lizec_crc32(uint32_t crc, const uint8_t *p, uint32_t len) {
	if (!crc_ready) lizec_crc32_init();
	crc ^= 0xFFFFFFFFu;
	while (len && ((uintptr_t)p & 7)) {
		crc = crc8tab[0][(crc ^ *p++) & 0xFF] ^ (crc >> 8);
		len--;
	}
	while (len >= 8) {
		uint64_t w;
		memcpy(&w, p, 8);
		w ^= crc;  /* little-endian host */
		crc = crc8tab[7][w & 0xff] ^ crc8tab[6][(w >> 8) & 0xff] ^
		      crc8tab[5][(w >> 16) & 0xff] ^ crc8tab[4][(w >> 24) & 0xff] ^
		      crc8tab[3][(w >> 32) & 0xff] ^ crc8tab[2][(w >> 40) & 0xff] ^
		      crc8tab[1][(w >> 48) & 0xff] ^ crc8tab[0][w >> 56];
		p += 8;
		len -= 8;
	}
	while (len) {
		crc = crc8tab[0][(crc ^ *p++) & 0xFF] ^ (crc >> 8);
		len--;
	}
	return crc ^ 0xFFFFFFFFu;
}

namespace {

uint32_t gf2_times(const uint32_t *mat, uint32_t vec) {
	uint32_t s = 0;
	for (int i = 0; vec; vec >>= 1, ++i)
		if (vec & 1) s ^= mat[i];
	return s;
}

void gf2_square(uint32_t *sq, const uint32_t *mat) {
	for (int i = 0; i < 32; ++i) sq[i] = gf2_times(mat, mat[i]);
}

}  // namespace

extern "C" uint32_t lizec_crc32_combine(uint32_t crc1, uint32_t crc2,
                                        uint32_t len2) {
	/* Matches the reference's table walk (crc.cc:207-224): advance crc1 by
	 * len2 zero bytes, xor crc2; len2==0 degenerates to crc1^crc2. */
	if (len2 == 0) return crc1 ^ crc2;
	uint32_t even[32], odd[32];
	odd[0] = 0xEDB88320u;
	for (int i = 1; i < 32; ++i) odd[i] = 1u << (i - 1);
	gf2_square(even, odd);
	gf2_square(odd, even);
	do {
		gf2_square(even, odd);
		if (len2 & 1) crc1 = gf2_times(even, crc1);
		len2 >>= 1;
		if (!len2) break;
		gf2_square(odd, even);
		if (len2 & 1) crc1 = gf2_times(odd, crc1);
		len2 >>= 1;
	} while (len2);
	return crc1 ^ crc2;
}

/* Partial-block CRC algebra — the crc.h:27-29 macros and hdd_write's
 * splice logic (hddspacemgr.cc:1952-2003) as first-class functions. */

/* crc.h:27: mycrc32_zeroblock — CRC after appending `zeros` zero bytes. */
extern "C" uint32_t lizec_crc32_zeroblock(uint32_t crc, uint32_t zeros) {
	return lizec_crc32_combine(crc ^ 0xFFFFFFFFu, 0xFFFFFFFFu, zeros);
}

/* crc.h:28: mycrc32_zeroexpanded — CRC of data followed by zeros. */
extern "C" uint32_t lizec_crc32_zeroexpanded(uint32_t crc, const uint8_t *block,
                                             uint32_t leng, uint32_t zeros) {
	return lizec_crc32_zeroblock(lizec_crc32(crc, block, leng), zeros);
}

/* crc.h:29: mycrc32_xorblocks — CRC of the byte-XOR of two equal-length
 * blocks from their CRCs (CRC is affine over GF(2)). */
extern "C" uint32_t lizec_crc32_xorblocks(uint32_t crc, uint32_t crcblock1,
                                          uint32_t crcblock2, uint32_t leng) {
	return crcblock1 ^ crcblock2 ^ lizec_crc32_zeroblock(crc, leng);
}

/* hdd_write's partial-write recombine (hddspacemgr.cc:1995-2003): CRC of a
 * block_len-byte block whose [offset, offset+size) range has CRC `crc`,
 * with precrc = CRC of [0, offset) and postcrc = CRC of the tail. */
extern "C" uint32_t lizec_crc32_splice(uint32_t precrc, uint32_t offset,
                                       uint32_t crc, uint32_t size,
                                       uint32_t postcrc, uint32_t block_len) {
	uint32_t combined;
	if (offset == 0) {
		return lizec_crc32_combine(crc, postcrc, block_len - size);
	}
	combined = lizec_crc32_combine(precrc, crc, size);
	if (offset + size < block_len)
		combined = lizec_crc32_combine(combined, postcrc,
		                               block_len - (offset + size));
	return combined;
}

/* crc.cc:235-243: sparse-file special case — a zero block whose cached
 * CRC is 0 gets the canonical empty-block CRC. */
extern "C" void lizec_recompute_crc_if_block_empty(const uint8_t *block,
                                                   uint32_t block_len,
                                                   uint32_t *crc) {
	if (*crc != 0) return;
	if (block[0] != 0 || memcmp(block, block + 1, block_len - 1) != 0) return;
	*crc = lizec_crc32_zeroblock(0, block_len);
}

/* The host checks of the write gate, shared by lizec_write_gate_host and
 * lizec_write_gate_batch (lizec_gpu.hip): hdd_write's own bounds
 * (hddspacemgr.cc:1912-1917) plus what an address table can get wrong. */
extern "C" int lizec_impl_write_gate_check(const lizec_write_op *ops,
                                           uint32_t n, uint32_t flags) {
	if (!ops || n == 0 || n > (1u << 24)) return LIZEC_EINVAL;
	if (flags & ~(uint32_t)LIZEC_GATE_SPARSE) return LIZEC_EINVAL;
	for (uint32_t i = 0; i < n; ++i) {
		const lizec_write_op &op = ops[i];
		if (op.size > 65536u || op.offset >= 65536u ||
		    op.offset + op.size > 65536u || op.reserved != 0)
			return LIZEC_EINVAL;
		if (op.size > 0 && op.data == 0) return LIZEC_EINVAL;
		const bool full = op.offset == 0 && op.size == 65536u;
		if (!full && op.block != 0 && op.stored == 0) return LIZEC_EINVAL;
	}
	return LIZEC_OK;
}

/* hdd_write's checks and CRC algebra (hddspacemgr.cc:1918-2001) over host
 * memory; see lizec.h. */
extern "C" int lizec_write_gate_host(const lizec_write_op *ops, uint32_t n,
                                     uint32_t flags, int32_t *status,
                                     uint32_t *newcrc) {
	if (!status || !newcrc) return LIZEC_EINVAL;
	int r = lizec_impl_write_gate_check(ops, n, flags);
	if (r != LIZEC_OK) return r;
	for (uint32_t i = 0; i < n; ++i) {
		const lizec_write_op &op = ops[i];
		status[i] = LIZEC_GATE_OK;
		newcrc[i] = 0;
		if (op.crc != lizec_crc32(0, (const uint8_t *)(uintptr_t)op.data,
		                          op.size)) {
			status[i] = LIZEC_GATE_BAD_DATA;
			continue;
		}
		if (op.offset == 0 && op.size == 65536u) {
			newcrc[i] = op.crc;
			continue;
		}
		const uint32_t end = op.offset + op.size, rest = 65536u - end;
		uint32_t pre, post;
		if (op.block == 0) {
			pre = lizec_crc32_zeroblock(0, op.offset);
			post = lizec_crc32_zeroblock(0, rest);
		} else {
			const uint8_t *b = (const uint8_t *)(uintptr_t)op.block;
			const uint8_t *p = (const uint8_t *)(uintptr_t)op.stored;
			pre = lizec_crc32(0, b, op.offset);
			post = lizec_crc32(0, b + end, rest);
			uint32_t have = lizec_crc32_splice(
			    pre, op.offset, lizec_crc32(0, b + op.offset, op.size),
			    op.size, post, 65536u);
			uint32_t stored = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) |
			                  ((uint32_t)p[2] << 8) | p[3];
			if (flags & LIZEC_GATE_SPARSE)
				lizec_recompute_crc_if_block_empty(b, 65536u, &stored);
			if (stored != have) {
				status[i] = LIZEC_GATE_BAD_BLOCK;
				continue;
			}
		}
		newcrc[i] = lizec_crc32_splice(pre, op.offset, op.crc, op.size, post,
		                               65536u);
	}
	return LIZEC_OK;
}

/* The host checks of the read gate, shared by lizec_read_gate_host and
 * lizec_read_gate_batch (lizec_gpu.hip): hdd_read's own bounds
 * (hddspacemgr.cc:1668-1671) plus what an address table can get wrong. */
extern "C" int lizec_impl_read_gate_check(const lizec_read_op *ops, uint32_t n,
                                          uint32_t flags) {
	if (!ops || n == 0 || n > (1u << 24)) return LIZEC_EINVAL;
	if (flags & ~(uint32_t)LIZEC_GATE_SPARSE) return LIZEC_EINVAL;
	for (uint32_t i = 0; i < n; ++i) {
		const lizec_read_op &op = ops[i];
		if (op.size == 0 || op.size > 65536u || op.offset >= 65536u ||
		    op.offset + op.size > 65536u)
			return LIZEC_EINVAL;
		if (op.out == 0) return LIZEC_EINVAL;
		if (op.block != 0 && op.stored == 0) return LIZEC_EINVAL;
	}
	return LIZEC_OK;
}

/* hdd_read over hdd_read_crc_and_block (hddspacemgr.cc:1525-1608,
 * :1709-1722) over host memory; see lizec.h. */
extern "C" int lizec_read_gate_host(const lizec_read_op *ops, uint32_t n,
                                    uint32_t flags, int32_t *status) {
	if (!status) return LIZEC_EINVAL;
	int r = lizec_impl_read_gate_check(ops, n, flags);
	if (r != LIZEC_OK) return r;
	for (uint32_t i = 0; i < n; ++i) {
		const lizec_read_op &op = ops[i];
		uint8_t *out = (uint8_t *)(uintptr_t)op.out;
		uint32_t crc;
		status[i] = LIZEC_GATE_OK;
		if (op.block == 0) {                                   /* :1535 */
			crc = lizec_crc32_zeroblock(0, op.size);
			memset(out + 4, 0, op.size);
		} else {
			const uint8_t *b = (const uint8_t *)(uintptr_t)op.block;
			const uint8_t *p = (const uint8_t *)(uintptr_t)op.stored;
			const uint32_t end = op.offset + op.size;
			const uint32_t mid = lizec_crc32(0, b + op.offset, op.size);
			const uint32_t have = lizec_crc32_splice(
			    lizec_crc32(0, b, op.offset), op.offset, mid, op.size,
			    lizec_crc32(0, b + end, 65536u - end), 65536u);
			uint32_t blk = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) |
			               ((uint32_t)p[2] << 8) | p[3];
			if ((flags & LIZEC_GATE_SPARSE) && blk == 0)       /* :1571 */
				lizec_recompute_crc_if_block_empty(b, 65536u, &blk);
			else if (blk != have)                              /* :1552 */
				status[i] = LIZEC_GATE_BAD_BLOCK;
			crc = (op.offset == 0 && op.size == 65536u) ? blk : mid;
			if (status[i] != LIZEC_GATE_OK) crc = 0;
			memcpy(out + 4, b + op.offset, op.size);
		}
		out[0] = (uint8_t)(crc >> 24);
		out[1] = (uint8_t)(crc >> 16);
		out[2] = (uint8_t)(crc >> 8);
		out[3] = (uint8_t)crc;
	}
	return LIZEC_OK;
}

/* C++-linkage aliases so a LizardFS build linking against common/crc.h's
 * mangled symbols (crc.h:25-31) resolves them from this library. */
uint32_t mycrc32(uint32_t crc, const uint8_t *block, uint32_t leng) {
	return lizec_crc32(crc, block, leng);
}
uint32_t mycrc32_combine(uint32_t crc1, uint32_t crc2, uint32_t leng2) {
	return lizec_crc32_combine(crc1, crc2, leng2);
}
void mycrc32_init(void) {
	lizec_crc32_init();
}

/* ------------------------------------------------------------------ */
/* XOR family host op (block_xor.h:33 drop-in; xor parity on GPU runs  */
/* through the EC kernel with all-ones coefficients)                   */
/* ------------------------------------------------------------------ */

extern "C" void lizec_blockxor(uint8_t *dest, const uint8_t *source,
                               size_t size) {
	size_t i = 0;
	for (; i + 8 <= size; i += 8) {
		uint64_t a, b;
		memcpy(&a, dest + i, 8);
		memcpy(&b, source + i, 8);
		a ^= b;
		memcpy(dest + i, &a, 8);
	}
	for (; i < size; ++i) dest[i] ^= source[i];
}

/* C++-linkage alias for the reference's mangled symbol (block_xor.h:33). */
void blockXor(uint8_t *dest, const uint8_t *source, size_t size) {
	lizec_blockxor(dest, source, size);
}

/* ------------------------------------------------------------------ */
/* Slice-type algebra (goal.h:108-119, slice_traits.h, chunk_part_type.h) */
/* ------------------------------------------------------------------ */

namespace {
constexpr int kECFirst = 10;               /* goal.h:118 */
constexpr int kECLast = kECFirst + 31 * 32 - 1;
constexpr int kMaxPartsCount = 64;         /* chunk_part_type.h:145 */
constexpr int64_t kBlockSize = 65536;      /* MFSBLOCKSIZE */
}

extern "C" int lizec_slice_type_ec(int k, int m) {
	if (k < 2 || k > 32 || m < 1 || m > 32) return -1;
	return 32 * (k - 2) + (m - 1) + kECFirst;   /* slice_traits.h:148-151 */
}

extern "C" int lizec_slice_is_ec(int t) {
	return t >= kECFirst && t <= kECLast;       /* slice_traits.h:67-70 */
}

extern "C" int lizec_slice_data_parts(int t) {
	if (!lizec_slice_is_ec(t)) return -1;
	return 2 + (t - kECFirst) / 32;             /* slice_traits.h:159-161 */
}

extern "C" int lizec_slice_parity_parts(int t) {
	if (!lizec_slice_is_ec(t)) return -1;
	return 1 + (t - kECFirst) % 32;             /* slice_traits.h:171-173 */
}

extern "C" int lizec_chunk_part_id(int slice_type, int part) {
	return slice_type * kMaxPartsCount + part;  /* chunk_part_type.h:170-174 */
}

extern "C" int lizec_chunk_part_slice_type(int id) {
	return id / kMaxPartsCount;
}

extern "C" int lizec_chunk_part_index(int id) {
	return id % kMaxPartsCount;
}

extern "C" int64_t lizec_chunk_part_length(int slice_type, int part,
                                           int64_t chunk_length) {
	/* slice_traits.h:332-349 */
	int k = lizec_slice_data_parts(slice_type);
	if (k < 0) return -1;
	if (k == 1) return chunk_length;
	int64_t full_stripe = chunk_length / (k * kBlockSize);
	int64_t base_len = full_stripe * kBlockSize;
	int64_t rest = chunk_length - base_len * k;
	int data_part_index = (part < k) ? part : 0;
	int64_t part_rest = rest - (int64_t)data_part_index * kBlockSize;
	if (part_rest < 0) part_rest = 0;
	if (part_rest > kBlockSize) part_rest = kBlockSize;
	return base_len + part_rest;
}

/* ------------------------------------------------------------------ */
/* Ragged EC batches: the block map (pure host, no GPU)               */
/* ------------------------------------------------------------------ */

extern "C" int64_t lizec_ragged_block_map(const uint32_t *dst_nblocks,
                                          int dests, int num_stripes,
                                          uint32_t *map,
                                          uint64_t cap_entries) {
	if (!dst_nblocks || dests < 1 || dests > 32 || num_stripes < 1)
		return LIZEC_EINVAL;
	uint64_t entries = 0;
	for (int s = 0; s < num_stripes; ++s) {
		uint32_t nb = 0;
		for (int l = 0; l < dests; ++l) {
			uint32_t n = dst_nblocks[(size_t)s * dests + l];
			if (n > 32768u) return LIZEC_EINVAL;
			if (n > nb) nb = n;
		}
		entries += nb;
	}
	/* one workgroup per 8 KiB tile at the most, in a 31-bit grid */
	if (entries * 8 > 0x7FFFFFFFull) return LIZEC_EINVAL;
	if (!map) return (int64_t)entries;
	if (entries > cap_entries) return LIZEC_EINVAL;
	for (int s = 0; s < num_stripes; ++s) {
		uint32_t nb = 0;
		for (int l = 0; l < dests; ++l)
			if (dst_nblocks[(size_t)s * dests + l] > nb)
				nb = dst_nblocks[(size_t)s * dests + l];
		for (uint32_t b = 0; b < nb; ++b) {
			*map++ = (uint32_t)s;
			*map++ = b;
		}
	}
	return (int64_t)entries;
}

/* ------------------------------------------------------------------ */
/* Batched chunk read: the checks and the host twin (pure host)       */
/* ------------------------------------------------------------------ */

/* The host checks of the chunk read, shared by lizec_chunk_read_host and
 * lizec_chunk_read_batch (lizec_gpu.hip).  Returns the entries of the row
 * map (one per (read, block row) that a range touches) or LIZEC_EINVAL;
 * *sbits / *dbits receive the OR of each side's stride and used addresses,
 * whose low bits choose the kernel form. */
extern "C" int64_t lizec_impl_chunk_read_check(
    int srcs, int rows, const uint8_t *gftbls, int ntables,
    const uint32_t *tbl_index, const uint64_t *src_dptrs,
    const uint32_t *src_nblocks, int view_parts, const uint8_t *col_map,
    const uint32_t *first_block, const uint32_t *block_count,
    const uint64_t *dst_dptrs, int num_reads, uint32_t src_block_stride,
    uint32_t dst_block_stride, uint64_t *sbits_out, uint64_t *dbits_out) {
	if (!src_dptrs || !src_nblocks || !col_map || !first_block ||
	    !block_count || !dst_dptrs)
		return LIZEC_EINVAL;
	if (srcs < 1 || srcs > 32 || rows < 0 || rows > 32 || view_parts < 1 ||
	    view_parts > 32 || num_reads < 1)
		return LIZEC_EINVAL;
	if (rows > 0) {
		if (!gftbls || ntables < 1 ||
		    (uint64_t)ntables * 32 * srcs * rows > (uint64_t)1 << 30)
			return LIZEC_EINVAL;
		if (tbl_index)
			for (int i = 0; i < num_reads; ++i)
				if (tbl_index[i] >= (uint32_t)ntables) return LIZEC_EINVAL;
	}
	if (src_block_stride < 65536u || dst_block_stride < 65536u)
		return LIZEC_EINVAL;
	const uint32_t ks = (uint32_t)view_parts;
	uint64_t sbits = src_block_stride, dbits = dst_block_stride;
	uint64_t entries = 0;
	for (int i = 0; i < num_reads; ++i) {
		const uint64_t *sp = src_dptrs + (size_t)i * srcs;
		const uint32_t *sn = src_nblocks + (size_t)i * srcs;
		const uint8_t *cm = col_map + (size_t)i * ks;
		/* the sources, by the ragged call's rules */
		for (int j = 0; j < srcs; ++j) {
			if (sn[j] > 32768u) return LIZEC_EINVAL;
			if (!sn[j]) continue;
			if (!sp[j]) return LIZEC_EINVAL;
			sbits |= sp[j];
		}
		const uint64_t first = first_block[i], count = block_count[i];
		if (count == 0 || first + count > 1048576u) return LIZEC_EINVAL;
		if (!dst_dptrs[i]) return LIZEC_EINVAL;
		dbits |= dst_dptrs[i];
		/* the column map: every value names something that exists, and no
		 * slot or table row stands for two columns */
		uint32_t slots_seen = 0, rows_seen = 0;
		for (uint32_t c = 0; c < ks; ++c) {
			const uint32_t v = cm[c];
			const bool req = count >= ks || (c + ks - first % ks) % ks < count;
			if (v == 0xFF) {
				if (req) return LIZEC_EINVAL;
			} else if (v >= 0x80) {
				const uint32_t r = v - 0x80;
				if (r >= (uint32_t)rows || ((rows_seen >> r) & 1))
					return LIZEC_EINVAL;
				rows_seen |= 1u << r;
			} else {
				if (v >= (uint32_t)srcs || ((slots_seen >> v) & 1))
					return LIZEC_EINVAL;
				slots_seen |= 1u << v;
				if (req && !sp[v]) return LIZEC_EINVAL;
			}
		}
		entries += (first + count - 1) / ks - first / ks + 1;
	}
	if ((sbits | dbits) & 3) return LIZEC_EINVAL;
	/* one workgroup per 8 KiB tile at the most, in a 31-bit grid */
	if (entries * 8 > 0x7FFFFFFFull) return LIZEC_EINVAL;
	if (sbits_out) *sbits_out = sbits;
	if (dbits_out) *dbits_out = dbits;
	return (int64_t)entries;
}

/* ChunkReader::readData over host memory, row by row: memcpy for the
 * columns a source backs, ec_encode_data over the present sources for the
 * lost ones; see lizec.h. */
static void chunk_read_host_run(
    int srcs, int rows, const uint8_t *gftbls, const uint32_t *tbl_index,
    const uint64_t *src_ptrs, const uint32_t *src_nblocks, int view_parts,
    const uint8_t *col_map, const uint32_t *first_block,
    const uint32_t *block_count, const uint64_t *dst_ptrs, int num_reads,
    uint32_t src_block_stride, uint32_t dst_block_stride) {
	const uint32_t ks = (uint32_t)view_parts;
	uint8_t tbl[32 * 32 * 32];   /* the lost rows over the present sources */
	for (int i = 0; i < num_reads; ++i) {
		const uint64_t *sp = src_ptrs + (size_t)i * srcs;
		const uint32_t *sn = src_nblocks + (size_t)i * srcs;
		const uint8_t *cm = col_map + (size_t)i * ks;
		const uint8_t *rt =
		    rows ? gftbls + (size_t)(tbl_index ? tbl_index[i] : 0) * 32 *
		                        srcs * rows
		         : nullptr;
		uint8_t *dst = (uint8_t *)(uintptr_t)dst_ptrs[i];
		const uint32_t first = first_block[i], end = first + block_count[i];
		for (uint32_t b = first / ks; b <= (end - 1) / ks; ++b) {
			const uint32_t c0 = b * ks;
			const uint32_t lo = first > c0 ? first - c0 : 0;
			const uint32_t hi = end - c0 < ks ? end - c0 : ks;
			uint8_t *lost[32];
			int lost_row[32], nl = 0;
			for (uint32_t c = lo; c < hi; ++c) {
				uint8_t *o = dst + (uint64_t)(c0 + c - first) * dst_block_stride;
				const uint32_t v = cm[c];
				if (v >= 0x80) {
					lost[nl] = o;
					lost_row[nl++] = (int)(v - 0x80);
				} else if (b < sn[v]) {
					memcpy(o, (const uint8_t *)(uintptr_t)sp[v] +
					              (uint64_t)b * src_block_stride, 65536);
				} else {
					memset(o, 0, 65536);
				}
			}
			if (!nl) continue;
			uint8_t *in[32];
			int np = 0;
			for (int j = 0; j < srcs; ++j) {
				if (b >= sn[j]) continue;
				for (int l = 0; l < nl; ++l)
					memcpy(tbl + ((size_t)l * srcs + np) * 32,
					       rt + ((size_t)lost_row[l] * srcs + j) * 32, 32);
				in[np++] = (uint8_t *)(uintptr_t)sp[j] +
				           (uint64_t)b * src_block_stride;
			}
			if (!np) {
				for (int l = 0; l < nl; ++l) memset(lost[l], 0, 65536);
				continue;
			}
			/* the table was filled at row pitch srcs; close it up to np */
			if (np < srcs)
				for (int l = 1; l < nl; ++l)
					memmove(tbl + (size_t)l * np * 32,
					        tbl + (size_t)l * srcs * 32, (size_t)np * 32);
			ec_encode_data(65536, np, nl, tbl, in, lost);
		}
	}
}

extern "C" int lizec_chunk_read_host(
    int srcs, int rows, const uint8_t *gftbls, int ntables,
    const uint32_t *tbl_index, const uint64_t *src_ptrs,
    const uint32_t *src_nblocks, int view_parts, const uint8_t *col_map,
    const uint32_t *first_block, const uint32_t *block_count,
    const uint64_t *dst_ptrs, int num_reads, uint32_t src_block_stride,
    uint32_t dst_block_stride) {
	int64_t entries = lizec_impl_chunk_read_check(
	    srcs, rows, gftbls, ntables, tbl_index, src_ptrs, src_nblocks,
	    view_parts, col_map, first_block, block_count, dst_ptrs, num_reads,
	    src_block_stride, dst_block_stride, nullptr, nullptr);
	if (entries < 0) return (int)entries;
	chunk_read_host_run(srcs, rows, gftbls, tbl_index, src_ptrs, src_nblocks,
	                    view_parts, col_map, first_block, block_count, dst_ptrs,
	                    num_reads, src_block_stride, dst_block_stride);
	return LIZEC_OK;
}

/* The verified read on the host: lizec_crc32 over the source blocks that
 * the read consumes, by the rule of csrc/read_verify.h, then the read. */
extern "C" int lizec_chunk_read_verified_host(
    int srcs, int rows, const uint8_t *gftbls, int ntables,
    const uint32_t *tbl_index, const uint64_t *src_ptrs,
    const uint32_t *src_nblocks, int view_parts, const uint8_t *col_map,
    const uint32_t *first_block, const uint32_t *block_count,
    const uint64_t *dst_ptrs, int num_reads, uint32_t src_block_stride,
    uint32_t dst_block_stride, const uint64_t *crc_ptrs,
    uint32_t crc_block_stride, uint32_t *bad_out) {
	if (!crc_ptrs || !bad_out || crc_block_stride < 4) return LIZEC_EINVAL;
	int64_t entries = lizec_impl_chunk_read_check(
	    srcs, rows, gftbls, ntables, tbl_index, src_ptrs, src_nblocks,
	    view_parts, col_map, first_block, block_count, dst_ptrs, num_reads,
	    src_block_stride, dst_block_stride, nullptr, nullptr);
	if (entries < 0) return (int)entries;
	const uint32_t ks = (uint32_t)view_parts;
	for (int i = 0; i < num_reads; ++i) {
		const uint64_t *sp = src_ptrs + (size_t)i * srcs;
		const uint64_t *cp = crc_ptrs + (size_t)i * srcs;
		const uint32_t *sn = src_nblocks + (size_t)i * srcs;
		const uint8_t *cm = col_map + (size_t)i * ks;
		const uint32_t first = first_block[i], end = first + block_count[i];
		uint32_t bad = 0;
		for (uint32_t b = first / ks; b <= (end - 1) / ks; ++b) {
			const uint32_t c0 = b * ks;
			const uint32_t lo = first > c0 ? first - c0 : 0;
			const uint32_t hi = end - c0 < ks ? end - c0 : ks;
			/* the slots whose column is requested; every present slot if a
			 * lost column is */
			uint32_t slots = 0;
			for (uint32_t c = lo; c < hi; ++c) {
				if (cm[c] >= 0x80) slots = 0xFFFFFFFFu;
				else slots |= 1u << cm[c];
			}
			for (int j = 0; j < srcs; ++j) {
				if (!((slots >> j) & 1) || !cp[j] || b >= sn[j]) continue;
				const uint8_t *q = (const uint8_t *)(uintptr_t)cp[j] +
				                   (uint64_t)b * crc_block_stride;
				const uint32_t want = ((uint32_t)q[0] << 24) |
				                      ((uint32_t)q[1] << 16) |
				                      ((uint32_t)q[2] << 8) | q[3];
				if (lizec_crc32(0, (const uint8_t *)(uintptr_t)sp[j] +
				                       (uint64_t)b * src_block_stride,
				                65536) != want)
					bad |= 1u << j;
			}
		}
		bad_out[i] = bad;
	}
	chunk_read_host_run(srcs, rows, gftbls, tbl_index, src_ptrs, src_nblocks,
	                    view_parts, col_map, first_block, block_count, dst_ptrs,
	                    num_reads, src_block_stride, dst_block_stride);
	return LIZEC_OK;
}

/* ------------------------------------------------------------------ */
/* Batched chunk write: the checks and the host twin (pure host)      */
/* ------------------------------------------------------------------ */

static_assert(sizeof(lizec_chunk_write) == 40, "lizec_chunk_write has padding");

/* The host checks of the chunk write, shared by lizec_chunk_write_host and
 * lizec_chunk_write_batch (lizec_gpu.hip).  Returns the (write, block row)
 * pairs that the ranges touch, or LIZEC_EINVAL.  *bits receives the OR of
 * every used address and stride, every `from` and every size (low bits 0:
 * the aligned kernel form); *tiles16 / *tiles8 the workgroups of a pass with
 * 16 KiB / 8 KiB tiles; *ncrc the CRCs the call writes. */
extern "C" int64_t lizec_impl_chunk_write_check(
    int rows, const uint8_t *gftbls, const lizec_chunk_write *writes,
    int num_writes, const uint64_t *fill_ptrs, const uint32_t *fill_nblocks,
    int view_parts, uint32_t fill_block_stride, const uint64_t *par_ptrs,
    uint64_t *bits_out, uint64_t *tiles16_out, uint64_t *tiles8_out,
    uint64_t *ncrc_out) {
	if (!gftbls || !writes || !fill_ptrs || !fill_nblocks || !par_ptrs)
		return LIZEC_EINVAL;
	if (num_writes < 1 || rows < 1 || rows > 32 || view_parts < 1 ||
	    view_parts > 32)
		return LIZEC_EINVAL;
	if (fill_block_stride < 65536u) return LIZEC_EINVAL;
	const uint32_t ks = (uint32_t)view_parts;
	uint64_t bits = 0, entries = 0, tiles16 = 0, tiles8 = 0, ncrc = 0;
	for (int i = 0; i < num_writes; ++i) {
		const lizec_chunk_write &w = writes[i];
		if (w.from >= w.to || w.to > 65536u) return LIZEC_EINVAL;
		const uint32_t size = w.to - w.from;
		const uint64_t first = w.first_block, count = w.block_count;
		if (count == 0 || first + count > 1048576u) return LIZEC_EINVAL;
		if (!w.data || (w.crcs & 3)) return LIZEC_EINVAL;
		const uint64_t touched = (first + count - 1) / ks - first / ks + 1;
		bits |= w.data | size | w.from;
		if (count > 1) {
			if (w.data_stride < size) return LIZEC_EINVAL;
			bits |= w.data_stride;
		}
		if (touched > 1) {
			if (w.par_stride < size) return LIZEC_EINVAL;
			bits |= w.par_stride;
		}
		const uint64_t *fp = fill_ptrs + (size_t)i * ks;
		const uint32_t *fn = fill_nblocks + (size_t)i * ks;
		for (uint32_t c = 0; c < ks; ++c) {
			if (fn[c] > 32768u) return LIZEC_EINVAL;
			if (!fn[c]) continue;
			if (!fp[c]) return LIZEC_EINVAL;
			bits |= fp[c] | fill_block_stride;
		}
		uint32_t wanted = 0;
		for (int r = 0; r < rows; ++r) {
			const uint64_t p = par_ptrs[(size_t)i * rows + r];
			if (!p) continue;
			++wanted;
			bits |= p;
		}
		if (!wanted && !w.crcs) return LIZEC_EINVAL;
		entries += touched;
		tiles16 += touched * ((size + 16383u) / 16384u);
		tiles8 += touched * ((size + 8191u) / 8192u);
		if (w.crcs) ncrc += count + touched * wanted;
	}
	/* the grids the passes launch (ec_chunks_for in lizec_gpu.hip): a last
	 * pass of up to 4 rows cuts 16 KiB tiles, every other pass 8 KiB ones */
	const int last = rows % 8 ? rows % 8 : 8;
	const bool use16 = last <= 4, use8 = rows > 8 || last > 4;
	if ((use16 && tiles16 > 0x7FFFFFFFull) || (use8 && tiles8 > 0x7FFFFFFFull))
		return LIZEC_EINVAL;
	/* crc32_ranges_kernel's bound */
	if (ncrc > ((uint64_t)1 << 24)) return LIZEC_EINVAL;
	if (bits_out) *bits_out = bits;
	if (tiles16_out) *tiles16_out = tiles16;
	if (tiles8_out) *tiles8_out = tiles8;
	if (ncrc_out) *ncrc_out = ncrc;
	return (int64_t)entries;
}

/* ChunkWriter::startOperation over host memory, row by row: the columns are
 * pointed at the new data, the fill or a block of zeros, ec_encode_data
 * computes the wanted parities over [from, to), lizec_crc32 the packets'
 * CRCs; see lizec.h. */
extern "C" int lizec_chunk_write_host(
    int rows, const uint8_t *gftbls, const lizec_chunk_write *writes,
    int num_writes, const uint64_t *fill_ptrs, const uint32_t *fill_nblocks,
    int view_parts, uint32_t fill_block_stride, const uint64_t *par_ptrs) {
	int64_t entries = lizec_impl_chunk_write_check(
	    rows, gftbls, writes, num_writes, fill_ptrs, fill_nblocks, view_parts,
	    fill_block_stride, par_ptrs, nullptr, nullptr, nullptr, nullptr);
	if (entries < 0) return (int)entries;
	lizec_crc32_init();
	const uint32_t ks = (uint32_t)view_parts;
	static const uint8_t zeros[65536] = {0};
	uint8_t tbl[32 * 32 * 32];   /* the wanted rows, closed up */
	for (int i = 0; i < num_writes; ++i) {
		const lizec_chunk_write &w = writes[i];
		const uint32_t size = w.to - w.from;
		const uint32_t first = w.first_block, end = first + w.block_count;
		const uint64_t *fp = fill_ptrs + (size_t)i * ks;
		const uint32_t *fn = fill_nblocks + (size_t)i * ks;
		const uint64_t *pp = par_ptrs + (size_t)i * rows;
		const uint8_t *data = (const uint8_t *)(uintptr_t)w.data;
		/* unused, and unchecked, for a single block */
		const uint64_t dstride = w.block_count > 1 ? w.data_stride : 0;
		uint32_t *crcs = (uint32_t *)(uintptr_t)w.crcs;
		int want_row[32], nw = 0;
		for (int r = 0; r < rows; ++r)
			if (pp[r]) {
				memcpy(tbl + (size_t)nw * ks * 32, gftbls + (size_t)r * ks * 32,
				       (size_t)ks * 32);
				want_row[nw++] = r;
			}
		if (crcs)
			for (uint32_t b = 0; b < w.block_count; ++b)
				crcs[b] = lizec_crc32(0, data + b * dstride, size);
		if (!nw) continue;
		const uint32_t r0 = first / ks;
		for (uint32_t b = r0; b <= (end - 1) / ks; ++b) {
			uint8_t *in[32], *out[32];
			for (uint32_t c = 0; c < ks; ++c) {
				const uint32_t cb = b * ks + c;
				if (cb >= first && cb < end)
					in[c] = (uint8_t *)data + (cb - first) * dstride;
				else if (b < fn[c])
					in[c] = (uint8_t *)(uintptr_t)fp[c] +
					        (uint64_t)b * fill_block_stride + w.from;
				else
					in[c] = (uint8_t *)zeros;
			}
			const uint64_t poff =
			    b > r0 ? (uint64_t)(b - r0) * w.par_stride : 0;
			for (int l = 0; l < nw; ++l)
				out[l] = (uint8_t *)(uintptr_t)pp[want_row[l]] + poff;
			ec_encode_data((int)size, (int)ks, nw, tbl, in, out);
			if (crcs)
				for (int l = 0; l < nw; ++l)
					crcs[w.block_count + (size_t)(b - r0) * rows + want_row[l]] =
					    lizec_crc32(0, out[l], size);
		}
	}
	return LIZEC_OK;
}

/* ------------------------------------------------------------------ */
/* Degraded chunk write: the composite table, the checks and the host */
/* twin (pure host)                                                   */
/* ------------------------------------------------------------------ */

/* One coefficient table over "new columns + old sources" for a row shape of
 * a slice with lost parts; see lizec.h.  coef[r][c], c < k, is G[r,c] for a
 * NEW column; coef[r][k + j] collects, for the part behind slot j, G[r,c] if
 * it is the readable fill column c, and G[r,c] * R[c,s] for every lost fill
 * column c that is rebuilt from it.  The products are folded before the
 * tables are expanded, so the table gives what rebuilding first and encoding
 * second gives, bit for bit. */
extern "C" int lizec_degraded_write_table(
    int k, int m, int is_xor, uint32_t new_mask, uint32_t have_mask,
    uint64_t avail_mask, const uint8_t *slot_part, int srcs, uint8_t *gftbl,
    uint32_t *use_mask) {
	if (k < 1 || k > MAXK || m < 1 || m > MAXM || srcs < 1 || srcs > 32)
		return LIZEC_EINVAL;
	if (!slot_part || !gftbl || !use_mask) return LIZEC_EINVAL;
	if (is_xor && m != 1) return LIZEC_EINVAL;
	const int nparts = k + m;
	const uint64_t all = nparts == 64 ? ~0ULL : (((uint64_t)1 << nparts) - 1);
	const uint32_t cols = k == 32 ? ~0u : ((1u << k) - 1);
	if ((new_mask & ~cols) || (have_mask & ~cols) || (avail_mask & ~all))
		return LIZEC_EINVAL;
	int slot_of[MAXP];
	for (int p = 0; p < nparts; ++p) slot_of[p] = -1;
	for (int j = 0; j < srcs; ++j) {
		if (slot_part[j] >= nparts || slot_of[slot_part[j]] >= 0)
			return LIZEC_EINVAL;
		slot_of[slot_part[j]] = j;
	}
	const uint32_t fill = have_mask & ~new_mask;
	const uint32_t lost = fill & ~(uint32_t)(avail_mask & cols);

	/* the generator: its parity rows are G */
	uint8_t rs_matrix[MAXP * MAXK];
	if (is_xor) {
		memset(rs_matrix, 0, sizeof rs_matrix);
		for (int c = 0; c < k; ++c) rs_matrix[c * k + c] = rs_matrix[k * k + c] = 1;
	} else if (m >= 5 || (m == 4 && k > 20)) {
		gf_gen_cauchy1_matrix(rs_matrix, nparts, k);
	} else {
		gf_gen_rs_matrix(rs_matrix, nparts, k);
	}
	const uint8_t *G = rs_matrix + (size_t)k * k;

	/* the rebuild of lost columns: the first k available parts, ascending
	 * (ec_read_plan.h:126-133); row c of decode_m gives data column c over
	 * them, by the inversion of lizec_rs_tables */
	int surv[MAXK];
	uint8_t decode_m[MAXK * MAXK];
	if (lost) {
		int ns = 0;
		for (int p = 0; p < nparts && ns < k; ++p)
			if ((avail_mask >> p) & 1) surv[ns++] = p;
		if (ns < k) return LIZEC_EINVAL;   /* not enough parts to read */
		uint64_t present = 0;
		for (int i = 0; i < k; ++i) {
			/* a data part without this block row is zeros: it needs no slot */
			const bool zeros = surv[i] < k && !((have_mask >> surv[i]) & 1);
			if (!zeros && slot_of[surv[i]] < 0) return LIZEC_EINVAL;
			present |= (uint64_t)1 << surv[i];
		}
		uint8_t work[MAXP * MAXK];
		select_rows(work, rs_matrix, nparts, k, present);
		if (gf_invert_matrix(work, decode_m, k) != 0) return LIZEC_ESINGULAR;
	}

	const int nc = k + srcs;
	uint8_t coef[MAXM * 64];
	memset(coef, 0, (size_t)m * nc);
	for (int c = 0; c < k; ++c) {
		const uint32_t bit = 1u << c;
		if (new_mask & bit) {
			for (int r = 0; r < m; ++r) coef[r * nc + c] = G[r * k + c];
		} else if (lost & bit) {
			for (int i = 0; i < k; ++i) {
				if (slot_of[surv[i]] < 0) continue;   /* zeros, see above */
				const int at = k + slot_of[surv[i]];
				for (int r = 0; r < m; ++r)
					coef[r * nc + at] ^=
					    gfmul(G[r * k + c], decode_m[c * k + i]);
			}
		} else if (fill & bit) {
			if (slot_of[c] < 0) return LIZEC_EINVAL;
			for (int r = 0; r < m; ++r)
				coef[r * nc + k + slot_of[c]] ^= G[r * k + c];
		}
	}
	/* a data part without this block row counts as zeros: never read */
	uint32_t mask = 0;
	for (int j = 0; j < srcs; ++j) {
		const int p = slot_part[j];
		bool used = false;
		for (int r = 0; r < m; ++r) {
			if (p < k && !((have_mask >> p) & 1)) coef[r * nc + k + j] = 0;
			used |= coef[r * nc + k + j] != 0;
		}
		if (used) mask |= 1u << j;
	}
	ec_init_tables(nc, m, coef, gftbl);
	*use_mask = mask;
	return LIZEC_OK;
}

/* The host checks of the degraded chunk write, shared by
 * lizec_chunk_write_degraded_host and lizec_chunk_write_degraded_batch
 * (lizec_gpu.hip); the outputs are those of lizec_impl_chunk_write_check. */
extern "C" int64_t lizec_impl_chunk_write_degraded_check(
    int rows, const uint8_t *gftbls, int ntables, const uint32_t *use_masks,
    const uint32_t *tbl_index, const lizec_chunk_write *writes, int num_writes,
    const uint64_t *old_ptrs, const uint32_t *old_nblocks, int srcs,
    int view_parts, uint32_t old_block_stride, const uint64_t *par_ptrs,
    uint64_t *bits_out, uint64_t *tiles16_out, uint64_t *tiles8_out,
    uint64_t *ncrc_out) {
	if (!gftbls || !use_masks || !tbl_index || !writes || !old_ptrs ||
	    !old_nblocks || !par_ptrs)
		return LIZEC_EINVAL;
	if (num_writes < 1 || rows < 1 || rows > 32 || view_parts < 1 ||
	    view_parts > 32 || srcs < 1 || srcs > 32 || ntables < 1)
		return LIZEC_EINVAL;
	if (old_block_stride < 65536u) return LIZEC_EINVAL;
	if (srcs < 32)
		for (int t = 0; t < ntables; ++t)
			if (use_masks[t] >> srcs) return LIZEC_EINVAL;
	const uint32_t ks = (uint32_t)view_parts;
	uint64_t bits = 0, entries = 0, tiles16 = 0, tiles8 = 0, ncrc = 0;
	for (int i = 0; i < num_writes; ++i) {
		const lizec_chunk_write &w = writes[i];
		if (w.from >= w.to || w.to > 65536u) return LIZEC_EINVAL;
		const uint32_t size = w.to - w.from;
		const uint64_t first = w.first_block, count = w.block_count;
		if (count == 0 || first + count > 1048576u) return LIZEC_EINVAL;
		if (!w.data || (w.crcs & 3)) return LIZEC_EINVAL;
		const uint64_t touched = (first + count - 1) / ks - first / ks + 1;
		bits |= w.data | size | w.from;
		if (count > 1) {
			if (w.data_stride < size) return LIZEC_EINVAL;
			bits |= w.data_stride;
		}
		if (touched > 1) {
			if (w.par_stride < size) return LIZEC_EINVAL;
			bits |= w.par_stride;
		}
		for (int t = 0; t < 3; ++t)
			if (tbl_index[(size_t)i * 3 + t] >= (uint32_t)ntables)
				return LIZEC_EINVAL;
		const uint64_t *op = old_ptrs + (size_t)i * srcs;
		const uint32_t *on = old_nblocks + (size_t)i * srcs;
		/* the slots that a table of a touched row may take; the others are
		 * never addressed, so neither refused nor part of the aligned form */
		uint32_t used = use_masks[tbl_index[(size_t)i * 3]];
		if (touched > 1) used |= use_masks[tbl_index[(size_t)i * 3 + 2]];
		if (touched > 2) used |= use_masks[tbl_index[(size_t)i * 3 + 1]];
		for (int j = 0; j < srcs; ++j) {
			if (on[j] > 32768u) return LIZEC_EINVAL;
			if (!on[j] || !((used >> j) & 1)) continue;
			if (!op[j]) return LIZEC_EINVAL;
			bits |= op[j] | old_block_stride;
		}
		uint32_t wanted = 0;
		for (int r = 0; r < rows; ++r) {
			const uint64_t p = par_ptrs[(size_t)i * rows + r];
			if (!p) continue;
			++wanted;
			bits |= p;
		}
		if (!wanted && !w.crcs) return LIZEC_EINVAL;
		entries += touched;
		tiles16 += touched * ((size + 16383u) / 16384u);
		tiles8 += touched * ((size + 8191u) / 8192u);
		if (w.crcs) ncrc += count + touched * wanted;
	}
	/* the grids the passes launch, as in lizec_impl_chunk_write_check */
	const int last = rows % 8 ? rows % 8 : 8;
	const bool use16 = last <= 4, use8 = rows > 8 || last > 4;
	if ((use16 && tiles16 > 0x7FFFFFFFull) || (use8 && tiles8 > 0x7FFFFFFFull))
		return LIZEC_EINVAL;
	if (ncrc > ((uint64_t)1 << 24)) return LIZEC_EINVAL;
	if (bits_out) *bits_out = bits;
	if (tiles16_out) *tiles16_out = tiles16;
	if (tiles8_out) *tiles8_out = tiles8;
	if (ncrc_out) *ncrc_out = ncrc;
	return (int64_t)entries;
}

/* lizec_chunk_write_host with the degraded call's source walk: per touched
 * row the ks + srcs candidates are pointed at the new data, an old slot that
 * is in the row's mask and has the block, or a block of zeros, and
 * ec_encode_data applies the row's table; see lizec.h. */
extern "C" int lizec_chunk_write_degraded_host(
    int rows, const uint8_t *gftbls, int ntables, const uint32_t *use_masks,
    const uint32_t *tbl_index, const lizec_chunk_write *writes, int num_writes,
    const uint64_t *old_ptrs, const uint32_t *old_nblocks, int srcs,
    int view_parts, uint32_t old_block_stride, const uint64_t *par_ptrs) {
	int64_t entries = lizec_impl_chunk_write_degraded_check(
	    rows, gftbls, ntables, use_masks, tbl_index, writes, num_writes,
	    old_ptrs, old_nblocks, srcs, view_parts, old_block_stride, par_ptrs,
	    nullptr, nullptr, nullptr, nullptr);
	if (entries < 0) return (int)entries;
	lizec_crc32_init();
	const uint32_t ks = (uint32_t)view_parts, nc = ks + (uint32_t)srcs;
	static const uint8_t zeros[65536] = {0};
	std::vector<uint8_t> tbl((size_t)32 * nc * 32);   /* wanted rows, closed up */
	for (int i = 0; i < num_writes; ++i) {
		const lizec_chunk_write &w = writes[i];
		const uint32_t size = w.to - w.from;
		const uint32_t first = w.first_block, end = first + w.block_count;
		const uint64_t *op = old_ptrs + (size_t)i * srcs;
		const uint32_t *on = old_nblocks + (size_t)i * srcs;
		const uint64_t *pp = par_ptrs + (size_t)i * rows;
		const uint8_t *data = (const uint8_t *)(uintptr_t)w.data;
		const uint64_t dstride = w.block_count > 1 ? w.data_stride : 0;
		uint32_t *crcs = (uint32_t *)(uintptr_t)w.crcs;
		int want_row[32], nw = 0;
		for (int r = 0; r < rows; ++r)
			if (pp[r]) want_row[nw++] = r;
		if (crcs)
			for (uint32_t b = 0; b < w.block_count; ++b)
				crcs[b] = lizec_crc32(0, data + b * dstride, size);
		if (!nw) continue;
		const uint32_t r0 = first / ks, r1 = (end - 1) / ks;
		for (uint32_t b = r0; b <= r1; ++b) {
			const uint32_t ti =
			    tbl_index[(size_t)i * 3 + (b == r0 ? 0 : b == r1 ? 2 : 1)];
			const uint32_t mask = use_masks[ti];
			const uint8_t *t = gftbls + (size_t)ti * rows * nc * 32;
			for (int l = 0; l < nw; ++l)
				memcpy(tbl.data() + (size_t)l * nc * 32,
				       t + (size_t)want_row[l] * nc * 32, (size_t)nc * 32);
			uint8_t *in[64], *out[32];
			for (uint32_t c = 0; c < ks; ++c) {
				const uint32_t cb = b * ks + c;
				in[c] = cb >= first && cb < end
				            ? (uint8_t *)data + (cb - first) * dstride
				            : (uint8_t *)zeros;
			}
			for (int j = 0; j < srcs; ++j)
				in[ks + j] = ((mask >> j) & 1) && b < on[j]
				                 ? (uint8_t *)(uintptr_t)op[j] +
				                       (uint64_t)b * old_block_stride + w.from
				                 : (uint8_t *)zeros;
			const uint64_t poff =
			    b > r0 ? (uint64_t)(b - r0) * w.par_stride : 0;
			for (int l = 0; l < nw; ++l)
				out[l] = (uint8_t *)(uintptr_t)pp[want_row[l]] + poff;
			ec_encode_data((int)size, (int)nc, nw, tbl.data(), in, out);
			if (crcs)
				for (int l = 0; l < nw; ++l)
					crcs[w.block_count + (size_t)(b - r0) * rows + want_row[l]] =
					    lizec_crc32(0, out[l], size);
		}
	}
	return LIZEC_OK;
}

/* ------------------------------------------------------------------ */
/* Ragged streaming rebuild: checks, stage cut and host twin          */
/* (pure host)                                                        */
/* ------------------------------------------------------------------ */

namespace {

constexpr uint64_t kReplBlock = 65536;          /* MFSBLOCKSIZE */
constexpr uint64_t kReplHddBlock = 65536 + 4;   /* chunk.h:40 kHddBlockSize */
constexpr uint64_t kReplStageDefault = (uint64_t)1 << 31;

/* Bytes of the image of `nb` blocks; 0 = nothing to emit. */
inline uint64_t repl_image_bytes(uint32_t nb, uint32_t header_size,
                                 uint32_t flags) {
	return (flags & LIZEC_REPL_INTERLEAVED) ? nb * kReplHddBlock
	                                        : header_size + nb * kReplBlock;
}

}  // namespace

/* Every argument check of lizec_replicate_run_ragged, shared with
 * lizec_replicate_ragged_host; see lizec.h. */
extern "C" int lizec_impl_replicate_ragged_check(
    int ic, int oc, const uint8_t *gftbls, int ntables,
    const uint32_t *tbl_index, const uint64_t *host_src,
    const uint32_t *src_nblocks, const uint64_t *host_src_crc,
    const uint8_t *sigs, uint32_t sig_len, uint32_t header_size,
    uint32_t crc_off, const uint64_t *host_dst, const uint32_t *dst_nblocks,
    int nchunks, uint64_t stage_bytes, uint32_t flags,
    const uint32_t *bad_out) {
	(void)sigs;   /* NULL leaves the signature block zero */
	if (!gftbls || !host_src || !src_nblocks || !host_dst || !dst_nblocks ||
	    nchunks < 1)
		return LIZEC_EINVAL;
	if (ic < 1 || ic > 32 || oc < 1 || oc > 32) return LIZEC_EINVAL;
	if (flags & ~LIZEC_REPL_INTERLEAVED) return LIZEC_EINVAL;
	if (stage_bytes > kReplStageDefault) return LIZEC_EINVAL;
	if (host_src_crc && !bad_out) return LIZEC_EINVAL;
	if (ntables < 1 || (uint64_t)ntables * 32 * ic * oc > (uint64_t)1 << 30)
		return LIZEC_EINVAL;
	if (tbl_index)
		for (int c = 0; c < nchunks; ++c)
			if (tbl_index[c] >= (uint32_t)ntables) return LIZEC_EINVAL;
	const size_t nsrc = (size_t)nchunks * ic, ndst = (size_t)nchunks * oc;
	for (size_t i = 0; i < nsrc; ++i) {
		if (src_nblocks[i] > 1024u) return LIZEC_EINVAL;
		if (src_nblocks[i] && !host_src[i]) return LIZEC_EINVAL;
	}
	uint32_t max_dst = 0;
	for (size_t i = 0; i < ndst; ++i) {
		if (dst_nblocks[i] > 1024u) return LIZEC_EINVAL;
		if (dst_nblocks[i] && !host_dst[i]) return LIZEC_EINVAL;
		if (dst_nblocks[i] > max_dst) max_dst = dst_nblocks[i];
	}
	/* a stage's block rows are one ragged EC batch (8 KiB tiles in a 31-bit
	 * grid); bounding the whole run bounds every stage */
	if ((uint64_t)nchunks * max_dst * 8 > 0x7FFFFFFFull &&
	    lizec_ragged_block_map(dst_nblocks, oc, nchunks, nullptr, 0) < 0)
		return LIZEC_EINVAL;
	if (!(flags & LIZEC_REPL_INTERLEAVED)) {
		/* the staged images start 16-aligned and their blocks, header_size
		 * in, are written with 16-byte vector accesses */
		if (header_size % 16 || sig_len > header_size ||
		    (uint64_t)crc_off + 4 * (uint64_t)max_dst > header_size)
			return LIZEC_EINVAL;
	}
	return LIZEC_OK;
}

extern "C" int64_t lizec_replicate_ragged_stages(
    int ic, int oc, const uint32_t *src_nblocks, const uint64_t *host_dst,
    const uint32_t *dst_nblocks, int nchunks, uint32_t header_size,
    uint32_t flags, uint64_t stage_bytes, uint32_t *stage_first,
    uint64_t cap) {
	if (!src_nblocks || !host_dst || !dst_nblocks || nchunks < 1 || ic < 1 ||
	    ic > 32 || oc < 1 || oc > 32 || (flags & ~LIZEC_REPL_INTERLEAVED) ||
	    stage_bytes > kReplStageDefault)
		return LIZEC_EINVAL;
	if (!stage_bytes) stage_bytes = kReplStageDefault;
	uint64_t stages = 0, sum = 0;
	for (int c = 0; c < nchunks; ++c) {
		uint64_t foot = 0;
		for (int j = 0; j < ic; ++j) {
			if (src_nblocks[(size_t)c * ic + j] > 1024u) return LIZEC_EINVAL;
			foot += src_nblocks[(size_t)c * ic + j] * kReplBlock;
		}
		for (int l = 0; l < oc; ++l) {
			const size_t n = (size_t)c * oc + l;
			if (dst_nblocks[n] > 1024u) return LIZEC_EINVAL;
			if (!host_dst[n]) continue;   /* not wanted: no image staged */
			foot += (repl_image_bytes(dst_nblocks[n], header_size, flags) +
			         15) & ~(uint64_t)15;
		}
		/* a chunk opens a stage if it is the first, or does not fit behind
		 * the ones the open stage holds */
		if (c == 0 || sum + foot > stage_bytes) {
			if (stage_first) {
				if (stages + 1 >= cap) return LIZEC_EINVAL;
				stage_first[stages] = (uint32_t)c;
			}
			++stages;
			sum = 0;
		}
		sum += foot;
	}
	if (stage_first) stage_first[stages] = (uint32_t)nchunks;
	return (int64_t)stages;
}

/* lizec_replicate_run_ragged on the host, chunk by chunk: lizec_crc32 over
 * every counted source block that has a CRC, ec_encode_data per block row
 * over the sources that have the row, lizec_crc32 over what it wrote. */
extern "C" int lizec_replicate_ragged_host(
    int ic, int oc, const uint8_t *gftbls, int ntables,
    const uint32_t *tbl_index, const uint64_t *host_src,
    const uint32_t *src_nblocks, const uint64_t *host_src_crc,
    const uint8_t *sigs, uint32_t sig_len, uint32_t header_size,
    uint32_t crc_off, const uint64_t *host_dst, const uint32_t *dst_nblocks,
    int nchunks, uint32_t flags, uint32_t *bad_out) {
	int r = lizec_impl_replicate_ragged_check(
	    ic, oc, gftbls, ntables, tbl_index, host_src, src_nblocks,
	    host_src_crc, sigs, sig_len, header_size, crc_off, host_dst,
	    dst_nblocks, nchunks, 0, flags, bad_out);
	if (r != LIZEC_OK) return r;
	lizec_crc32_init();
	const bool il = (flags & LIZEC_REPL_INTERLEAVED) != 0;
	const uint64_t data_off = il ? 4 : header_size;
	const uint64_t coff = il ? 0 : crc_off;
	const uint64_t bstride = il ? kReplHddBlock : kReplBlock;
	const uint64_t cstride = il ? kReplHddBlock : 4;
	std::vector<uint8_t> tbl((size_t)32 * 32 * 32);   /* wanted rows, closed up */
	for (int c = 0; c < nchunks; ++c) {
		const uint64_t *sp = host_src + (size_t)c * ic;
		const uint32_t *sn = src_nblocks + (size_t)c * ic;
		const uint64_t *dp = host_dst + (size_t)c * oc;
		const uint32_t *dn = dst_nblocks + (size_t)c * oc;
		if (bad_out) {
			uint32_t bad = 0;
			for (int j = 0; host_src_crc && j < ic; ++j) {
				const uint8_t *q =
				    (const uint8_t *)(uintptr_t)host_src_crc[(size_t)c * ic + j];
				if (!q) continue;
				for (uint32_t b = 0; b < sn[j]; ++b, q += 4) {
					const uint32_t want = ((uint32_t)q[0] << 24) |
					                      ((uint32_t)q[1] << 16) |
					                      ((uint32_t)q[2] << 8) | q[3];
					if (lizec_crc32(0, (const uint8_t *)(uintptr_t)sp[j] +
					                       b * kReplBlock, 65536) != want)
						bad |= 1u << j;
				}
			}
			bad_out[c] = bad;
		}
		const uint8_t *t =
		    gftbls + (size_t)(tbl_index ? tbl_index[c] : 0) * 32 * ic * oc;
		uint32_t rows = 0;
		for (int l = 0; l < oc; ++l) {
			if (!dp[l]) continue;
			if (dn[l] > rows) rows = dn[l];
			if (il) continue;
			uint8_t *img = (uint8_t *)(uintptr_t)dp[l];
			memset(img, 0, header_size);
			if (sigs && sig_len)
				memcpy(img, sigs + ((size_t)c * oc + l) * sig_len, sig_len);
		}
		for (uint32_t b = 0; b < rows; ++b) {
			uint8_t *in[32], *out[32];
			int row[32], np = 0, nw = 0;
			for (int l = 0; l < oc; ++l)
				if (b < dn[l]) {
					row[nw] = l;
					out[nw++] = (uint8_t *)(uintptr_t)dp[l] + data_off +
					            b * bstride;
				}
			for (int j = 0; j < ic; ++j) {
				if (b >= sn[j]) continue;
				for (int l = 0; l < nw; ++l)
					memcpy(tbl.data() + ((size_t)l * ic + np) * 32,
					       t + ((size_t)row[l] * ic + j) * 32, 32);
				in[np++] = (uint8_t *)(uintptr_t)sp[j] + b * kReplBlock;
			}
			if (!np) {
				for (int l = 0; l < nw; ++l) memset(out[l], 0, 65536);
			} else {
				/* the table was filled at row pitch ic; close it up to np */
				if (np < ic)
					for (int l = 1; l < nw; ++l)
						memmove(tbl.data() + (size_t)l * np * 32,
						        tbl.data() + (size_t)l * ic * 32,
						        (size_t)np * 32);
				ec_encode_data(65536, np, nw, tbl.data(), in, out);
			}
			for (int l = 0; l < nw; ++l) {
				const uint32_t crc = lizec_crc32(0, out[l], 65536);
				uint8_t *q = (uint8_t *)(uintptr_t)dp[row[l]] + coff +
				             b * cstride;
				q[0] = (uint8_t)(crc >> 24);
				q[1] = (uint8_t)(crc >> 16);
				q[2] = (uint8_t)(crc >> 8);
				q[3] = (uint8_t)crc;
			}
		}
	}
	return LIZEC_OK;
}
