/* lizec.h — C ABI of the MI355X-native LizardFS erasure-coding engine.
 *
 * This is the drop-in boundary for the LizardFS chunkserver/client EC hot
 * path.  The reference already swaps EC backends at exactly this seam: its
 * reed_solomon.h:27-31 compiles against either Intel ISA-L's
 * <isa-l/erasure_code.h> or the in-tree common/galois_field.h:35-88 — both
 * expose the five functions below.  liblizec.so exports them with the same
 * names and semantics (extern "C", ISA-L calling convention), so a LizardFS
 * build configured for ISA-L links against this library unchanged.  The CRC
 * surface mirrors common/crc.h:25-31 (also exported with C++ linkage from
 * the library so the reference's mangled references resolve).
 *
 * On top of the per-call surface sits the batched GPU engine (lizec_engine,
 * lizec_*_batch): the product proper.  Per-64KiB-call granularity cannot
 * feed a GPU, so the engine takes batches of stripes of device-resident
 * parts; the host-side matrix algebra (reference reed_solomon.h:163-358)
 * stays on the CPU exactly as in the reference.
 *
 * Ownership/threading: caller owns every buffer; no function retains state
 * except the engine object.  The per-call functions are pure and
 * thread-safe (matching bgjobs-worker concurrency in the reference,
 * network_main_thread.cc:230-234).  One engine is safe to use from several
 * threads at once as long as concurrent calls pass distinct streams (each
 * stream has its own call scratch); calls on one stream must not overlap.
 *
 * Error convention: 0 = success; negative = error (see LIZEC_E*).  The GF
 * layer itself only signals singular matrices, like the reference
 * (galois_field_isal.cc:87-139 returns -1).
 */
#ifndef LIZEC_H
#define LIZEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ */
/* ISA-L-shaped surface — drop-in for common/galois_field.h:35-88.    */
/* GF(2^8), polynomial 0x11D (galois_coeff.h:30-32).                  */
/* ------------------------------------------------------------------ */

/* (k+m) x k Vandermonde-style generator matrix; identity on top.
 * Replaces gf_gen_rs_matrix (galois_field.h:35, galois_field_isal.cc:53). */
void gf_gen_rs_matrix(uint8_t *a, int m, int k);

/* (k+m) x k Cauchy matrix (1/(i^j)); identity on top.
 * Replaces gf_gen_cauchy1_matrix (galois_field.h:48, galois_field_isal.cc:71). */
void gf_gen_cauchy1_matrix(uint8_t *a, int m, int k);

/* Gauss-Jordan inversion in GF(2^8).  Mutates in_mat.  -1 if singular.
 * Replaces gf_invert_matrix (galois_field.h:58, galois_field_isal.cc:87). */
int gf_invert_matrix(uint8_t *in_mat, uint8_t *out_mat, const int n);

/* Expand rows*k coefficients into 32-byte lo/hi-nibble product tables
 * (tbl[i]=c*i, tbl[16+i]=c*(i<<4)); layout [row][col][32].
 * Replaces ec_init_tables (galois_field.h:71, galois_field_isal.cc:246). */
void ec_init_tables(int k, int rows, uint8_t *a, uint8_t *g_tbls);

/* Host scalar encode: dest[l][i] = XOR_j tbl(l,j)[src[j][i]].  This is the
 * reference's per-64KiB-block CPU entry point (galois_field.h:88,
 * galois_field_encode.cc:28-225); kept for drop-in completeness and for the
 * host-side matrixMultiply.  The measured product path is the batched GPU
 * engine below — this function never runs inside it. */
void ec_encode_data(int len, int srcs, int dests, uint8_t *v, uint8_t **src,
                    uint8_t **dest);

/* ------------------------------------------------------------------ */
/* CRC surface — drop-in for common/crc.h:25-31.                      */
/* Reflected CRC-32, poly 0xEDB88320, zlib-compatible.                */
/* ------------------------------------------------------------------ */

uint32_t lizec_crc32(uint32_t crc, const uint8_t *block, uint32_t leng);
uint32_t lizec_crc32_combine(uint32_t crc1, uint32_t crc2, uint32_t leng2);
void lizec_crc32_init(void);

/* Partial-block CRC algebra (crc.h:27-29 macros + hdd_write's splice,
 * hddspacemgr.cc:1952-2003) — byte-range writes without re-hashing. */
uint32_t lizec_crc32_zeroblock(uint32_t crc, uint32_t zeros);
uint32_t lizec_crc32_zeroexpanded(uint32_t crc, const uint8_t *block,
                                  uint32_t leng, uint32_t zeros);
uint32_t lizec_crc32_xorblocks(uint32_t crc, uint32_t crcblock1,
                               uint32_t crcblock2, uint32_t leng);
uint32_t lizec_crc32_splice(uint32_t precrc, uint32_t offset, uint32_t crc,
                            uint32_t size, uint32_t postcrc,
                            uint32_t block_len);
void lizec_recompute_crc_if_block_empty(const uint8_t *block,
                                        uint32_t block_len, uint32_t *crc);

/* Host byte-XOR (xor-goal parity building block; also exported with the
 * C++ mangling of the reference's blockXor, common/block_xor.h:33).
 * GPU xor parity/recovery runs through the EC kernel with all-ones
 * coefficient tables (lizardfs_amd/xor.py). */
void lizec_blockxor(uint8_t *dest, const uint8_t *source, size_t size);

/* ------------------------------------------------------------------ */
/* Reed-Solomon table builders — host-side restatement of             */
/* ReedSolomon<32,32> (reed_solomon.h:41-373).                        */
/* Parts indexed 0..k+m-1: data 0..k-1, parity k..k+m-1               */
/* (slice_traits.h:183-197).  Matrix: Cauchy iff m>=5 || (m==4 &&     */
/* k>20), else Vandermonde (reed_solomon.h:168).                      */
/* ------------------------------------------------------------------ */

enum {
	LIZEC_EINVAL = -2,
	LIZEC_ESINGULAR = -1,   /* decode matrix not invertible */
	LIZEC_OK = 0,
	LIZEC_ENOGPU = -3,
	LIZEC_EHIP = -4,
	LIZEC_ENOMEM = -5,
};

/* Expanded gf tables for ReedSolomon::recover (reed_solomon.h:87-121):
 *  present_mask: parts NOT erased (bit i = part i available)
 *  nonnull_mask: available parts whose buffer is non-NULL (NULL = zeros,
 *                reed_solomon.h:79); must be a subset of present_mask
 *  needed_mask : erased parts to reconstruct (subset of ~present_mask)
 * gftbls must hold 32 * popcount(nonnull) * popcount(needed) bytes.
 * Outputs the number of inputs (surviving non-NULL parts, ascending part
 * order) and outputs (needed parts, ascending part order).
 * Encode is the special case present=nonnull=data parts,
 * needed=all m parities (reed_solomon.h:134-155). */
int lizec_rs_tables(int k, int m, uint64_t present_mask, uint64_t nonnull_mask,
                    uint64_t needed_mask, uint8_t *gftbls, int *in_count,
                    int *out_count);

/* Convenience: encode tables for all m parities from all k data parts. */
int lizec_rs_encode_tables(int k, int m, uint8_t *gftbls /* 32*k*m */);

/* ------------------------------------------------------------------ */
/* Slice-type algebra — mirror of slice_traits.h / goal.h:108-119.    */
/* EC(k,m) slice type = 32*(k-2) + (m-1) + 10  (slice_traits.h:148).  */
/* ------------------------------------------------------------------ */

int lizec_slice_type_ec(int data_parts, int parity_parts);
int lizec_slice_is_ec(int slice_type);
int lizec_slice_data_parts(int slice_type);    /* k */
int lizec_slice_parity_parts(int slice_type);  /* m */
/* ChunkPartType packing: id = type*64 + part (chunk_part_type.h:145,170). */
int lizec_chunk_part_id(int slice_type, int part);
int lizec_chunk_part_slice_type(int id);
int lizec_chunk_part_index(int id);
/* chunkLengthToChunkPartLength (slice_traits.h:332-349); block = 64 KiB. */
int64_t lizec_chunk_part_length(int slice_type, int part, int64_t chunk_length);

/* ------------------------------------------------------------------ */
/* The batched GPU engine (the product).                              */
/* All device pointers are HIP device addresses on the engine's       */
/* device; `stream` is a hipStream_t (NULL = engine's own stream).    */
/* Calls are asynchronous on that stream.  Fails with LIZEC_ENOGPU    */
/* if no MI355X is present — there is no CPU fallback.                */
/* ------------------------------------------------------------------ */

typedef struct lizec_engine lizec_engine;

int lizec_gpu_count(void);
int lizec_engine_create(lizec_engine **out, int device_id);
void lizec_engine_destroy(lizec_engine *e);
int lizec_engine_sync(lizec_engine *e);

/* Batched EC encode/decode over device-resident stripes.  All stripes in a
 * batch share (srcs, dests, part_len).  This entry point also shares one
 * gftbls across the batch — the reference likewise reuses one cached table
 * per (erasure pattern, k, m) (reed_solomon.h:194-198); batches whose
 * stripes carry different erasure patterns go through
 * lizec_ec_encode_batch_multi below.
 *  part_len : bytes per part
 *  gftbls   : HOST pointer, 32*srcs*dests bytes (from lizec_rs_tables)
 *  src_dptrs: HOST array of num_stripes*srcs device addresses
 *             (stripe-major: stripe s, input j at [s*srcs + j])
 *  dst_dptrs: HOST array of num_stripes*dests device addresses
 * Every part address must be 16-byte aligned (the kernels move parts in
 * 16-byte vectors), and part_len a multiple of 16; otherwise the call
 * returns LIZEC_EINVAL from the host and enqueues nothing.  The same rule
 * holds for the plan and multi-table forms below, where a destination
 * address of 0 stays legal.
 * Covers encode (a1/a6: chunk_writer.cc:365-402), degraded-read decode
 * (ec_read_plan.h:113-146) and replicator recovery
 * (chunk_replicator.cc:139-196) — all three reduce to ec_encode_data with
 * different tables. */
int lizec_ec_encode_batch(lizec_engine *e, uint64_t part_len, int srcs,
                          int dests, const uint8_t *gftbls,
                          const uint64_t *src_dptrs, const uint64_t *dst_dptrs,
                          int num_stripes, void *stream);

/* Prepared batches ("plans", after the reference's read-plan/matrix-cache
 * structure, read_plan.h + reed_solomon.h:194-198): device-resident tables
 * and pointer arrays built once, then run repeatedly with no host->device
 * traffic.  Same arguments as lizec_ec_encode_batch. */
typedef struct lizec_plan lizec_plan;
int lizec_ec_plan_create(lizec_engine *e, uint64_t part_len, int srcs,
                         int dests, const uint8_t *gftbls,
                         const uint64_t *src_dptrs, const uint64_t *dst_dptrs,
                         int num_stripes, lizec_plan **out);
int lizec_ec_plan_run(lizec_plan *p, void *stream);
void lizec_ec_plan_destroy(lizec_plan *p);

/* Batched EC decode with a coefficient table PER STRIPE: one call (one
 * launch per pass of 8 destinations) covers a batch of mixed erasure
 * patterns — a rebuild after a disk loss (chunk_replicator.cc:139-196,
 * where the lost disk held a different part of every chunk) or a batch of
 * degraded reads (ec_read_plan.h:113-146, one pattern per read operation).
 *  gftbls   : HOST pointer, ntables tables of 32*srcs*dests bytes each
 *             (ISA-L layout, from lizec_rs_tables; a stripe that needs
 *             fewer than `dests` outputs pads its table with zero rows)
 *  ntables  : >= 1, and ntables*32*srcs*dests <= 2^30 bytes
 *  tbl_index: HOST array, num_stripes entries, each < ntables; checked on
 *             the host before anything is enqueued (LIZEC_EINVAL)
 *  dst_dptrs: as above, but address 0 = do not write that output
 * Everything else (srcs, dests, part_len uniform over the batch; stream
 * and thread contract) is as for lizec_ec_encode_batch. */
int lizec_ec_encode_batch_multi(lizec_engine *e, uint64_t part_len, int srcs,
                                int dests, const uint8_t *gftbls, int ntables,
                                const uint32_t *tbl_index,
                                const uint64_t *src_dptrs,
                                const uint64_t *dst_dptrs, int num_stripes,
                                void *stream);

/* Plan form of the above; run/destroy it with lizec_ec_plan_run and
 * lizec_ec_plan_destroy. */
int lizec_ec_plan_create_multi(lizec_engine *e, uint64_t part_len, int srcs,
                               int dests, const uint8_t *gftbls, int ntables,
                               const uint32_t *tbl_index,
                               const uint64_t *src_dptrs,
                               const uint64_t *dst_dptrs, int num_stripes,
                               lizec_plan **out);

/* Batched EC encode/decode over parts stored as 64 KiB blocks at a fixed
 * stride, at addresses that need only be 4-byte aligned — the layout of an
 * INTERLEAVED-format chunk part (kHddBlockSize = 65540, chunk.h:40: block
 * b's data at 4 + 65540*b, so its alignment cycles through 4, 8, 12, 0
 * mod 16).  Survivors can be read from such images and parts rebuilt into
 * them in place.
 *  nblocks  : 64 KiB blocks per part (part length = nblocks*65536 <= 2^31)
 *  gftbls, src_dptrs, dst_dptrs, num_stripes: as for lizec_ec_encode_batch,
 *             an address being that of block 0's DATA (the caller folds a
 *             header, or an image's leading 4 bytes, into it)
 *  src_block_stride / dst_block_stride: block b of a part lies at
 *             address + b*stride; >= 65536, one value per side
 * Only bytes inside [block, block + 65536) are read or written: whatever
 * lies between two destination blocks (the CRC slots) survives the call.
 * Returns LIZEC_EINVAL from the host, with nothing enqueued, if an address
 * or stride is not a multiple of 4, a stride is below 65536, nblocks is 0
 * or nblocks*65536 > 2^31, srcs or dests is outside 1..32, an address is 0,
 * or num_stripes*nblocks*8 (the batch counted in 8 KiB tiles, one
 * workgroup each) exceeds 2^31-1.
 * A side whose addresses and stride are all multiples of 16 keeps the
 * aligned vector accesses; with both sides so and both strides 65536 the
 * call is lizec_ec_encode_batch at part_len = nblocks*65536.  Stream and
 * thread contract as for the other batch calls. */
int lizec_ec_encode_batch_strided(lizec_engine *e, uint32_t nblocks, int srcs,
                                  int dests, const uint8_t *gftbls,
                                  const uint64_t *src_dptrs,
                                  const uint64_t *dst_dptrs, int num_stripes,
                                  uint32_t src_block_stride,
                                  uint32_t dst_block_stride, void *stream);

/* Batched EC encode/decode over parts of DIFFERENT lengths: the strided
 * call above with a block count per source and per destination of every
 * stripe, and a coefficient table per stripe.  A chunk is 1..1024 blocks
 * and only a full one gives its parts a common length — data part p of a
 * chunk of n blocks has (n + k - p - 1) / k blocks (slice_traits.h:311-316)
 * — so one call rebuilds chunks of any mix of lengths and erasure patterns,
 * straight into images of either on-disk format
 * (ChunkReplicator::replicate, chunk_replicator.cc:142-145).
 *  gftbls, ntables, tbl_index: as for lizec_ec_encode_batch_multi;
 *             tbl_index may be NULL = every stripe uses table 0
 *  src_dptrs / src_nblocks: HOST arrays [num_stripes][srcs]: address of
 *             block 0's data and number of blocks of every source.  Source
 *             j takes part in block b iff b < its count; beyond that it
 *             counts as zeros and no byte of it is read — the reference's
 *             NULL-part rule (reed_solomon.h:79) per block.  An address
 *             whose count is 0 is never used and may be 0.
 *  dst_dptrs / dst_nblocks: HOST arrays [num_stripes][dests], likewise:
 *             destination l is written for block b iff b < its count; a
 *             block that no source covers is written as zeros.  A stripe
 *             whose destination counts are all 0 is legal and costs nothing.
 *  src_block_stride / dst_block_stride: as for the strided call
 * Only bytes inside the counted blocks are read or written.
 * Returns LIZEC_EINVAL from the host, with nothing enqueued, if a stride or
 * a used address is not a multiple of 4, a stride is below 65536, srcs or
 * dests is outside 1..32, a count exceeds 32768, a nonzero count comes with
 * address 0, a tbl_index entry is >= ntables, ntables is outside the limits
 * of the multi call, no destination has any block, or the block rows of the
 * batch (lizec_ragged_block_map) times 8 exceed 2^31-1.
 * A side whose stride and used addresses are all multiples of 16 keeps the
 * aligned vector accesses.  There is no plan form.  Stream and thread
 * contract as for the other batch calls. */
int lizec_ec_encode_batch_ragged(lizec_engine *e, int srcs, int dests,
                                 const uint8_t *gftbls, int ntables,
                                 const uint32_t *tbl_index,
                                 const uint64_t *src_dptrs,
                                 const uint32_t *src_nblocks,
                                 const uint64_t *dst_dptrs,
                                 const uint32_t *dst_nblocks, int num_stripes,
                                 uint32_t src_block_stride,
                                 uint32_t dst_block_stride, void *stream);

/* Batched EC over parts cut from a CHUNK VIEW: the ragged call above with
 * the chunk's data, held in another slice type, as its source side.  This is
 * how SliceRecoveryPlanner builds a part that its own slice cannot give
 * (slice_recovery_planner.h:85-204), the path of every chunk when a goal
 * changes (2 copies -> ec(8,2), ec(3,2) -> ec(8,2)): the chunk is read as
 * consecutive blocks (chunk_read_planner.h:36-58), a data part of the target
 * is every row_cols-th of them (kRecoverDataPart, :41-55), a parity part is
 * computed over rows of row_cols consecutive ones (kRecoverParityPart,
 * ec_read_plan.h:38-66, xor_read_plan.h:39).
 *  gftbls, ntables, tbl_index, dst_dptrs, dst_nblocks, strides: as for
 *             lizec_ec_encode_batch_ragged
 *  view_dptrs : HOST array [num_stripes][view_parts]: address of block 0's
 *             data of every data part of the SOURCE slice, in view-column
 *             order (standard: the copy; xorN: parts 1..N; ec(k,m): parts
 *             0..k-1)
 *  view_parts : data parts of the source slice, 1..32; one value per call
 *  chunk_blocks: HOST array [num_stripes]: n, the blocks of the chunk.
 *             Chunk block c < n is the 64 KiB at
 *             view[c % view_parts] + (c / view_parts) * src_block_stride;
 *             blocks from n on count as zeros and no byte of them is read.
 *             View address p is used iff p < n; an unused one may be 0.
 *  row_cols   : data parts of the TARGET slice, 1..32
 *  src_col0   : HOST array [num_stripes], or NULL = all 0.  In block row b
 *             source j (the table's column j) is chunk block
 *             b*row_cols + src_col0[s] + j.  A parity target has column 0 and
 *             srcs = row_cols; a data target has its part index, srcs = 1 and
 *             a table of coefficient 1.
 * A destination block that no source reaches is written as zeros.  Whole
 * chunks only: there is no starting row.
 * Returns LIZEC_EINVAL from the host, with nothing enqueued, for everything
 * the ragged call refuses about tables, destinations and strides, and if
 * view_parts or row_cols is outside 1..32, src_col0[s] + srcs > row_cols,
 * chunk_blocks[s] is 0 or above 1048576, or a used view address is 0 or not
 * a multiple of 4.
 * The source side keeps the aligned vector accesses if its stride and used
 * view addresses are all multiples of 16.  There is no plan form.  Stream
 * and thread contract as for the other batch calls. */
int lizec_ec_encode_batch_view(lizec_engine *e, int srcs, int dests,
                               const uint8_t *gftbls, int ntables,
                               const uint32_t *tbl_index,
                               const uint64_t *view_dptrs, int view_parts,
                               const uint32_t *chunk_blocks, int row_cols,
                               const uint32_t *src_col0,
                               const uint64_t *dst_dptrs,
                               const uint32_t *dst_nblocks, int num_stripes,
                               uint32_t src_block_stride,
                               uint32_t dst_block_stride, void *stream);

/* The block map of a ragged batch; pure host code, needs no GPU.  One
 * entry (stripe, block) per 64 KiB block row: stripe s contributes blocks
 * 0 .. max_l dst_nblocks[s][l] - 1, stripe-major, ascending.
 *  map        : 2 words per entry, or NULL to count only
 *  cap_entries: room in map, in entries
 * Returns the entry count (0 if no destination has a block), or
 * LIZEC_EINVAL if dests is outside 1..32, num_stripes < 1, a count exceeds
 * 32768, the entries do not fit cap_entries, or entries*8 > 2^31-1 (the
 * batch counted in 8 KiB tiles, one workgroup each). */
int64_t lizec_ragged_block_map(const uint32_t *dst_nblocks, int dests,
                               int num_stripes, uint32_t *map,
                               uint64_t cap_entries);

/* Batched chunk READ — ChunkReader::readData (chunk_reader.cc:85-131) for
 * num_reads requests at once: chunk blocks [first_block, first_block +
 * block_count) gathered from the parts of one slice, whose data parts
 * interleave the chunk round-robin (ChunkReadPlanner,
 * chunk_read_planner.h:86-162), the blocks of lost parts rebuilt on the way
 * (ECReadPlan::recoverParts, ec_read_plan.h:113-146;
 * XorReadPlan::postProcessRead, xor_read_plan.h:77-126) and everything put
 * into chunk order (BlockConverter, chunk_read_planner.h:36-58).  One read
 * is one readData request on one chunk.
 *  srcs       : source slots per read, 1..32
 *  rows       : rows of a coefficient table, 0..32: the most columns that a
 *             read of the call rebuilds.  0 makes the call a pure gather —
 *             BlockConverter on the device for a healthy slice; gftbls,
 *             ntables and tbl_index are then ignored and may be NULL / 0.
 *  gftbls, ntables, tbl_index: as for lizec_ec_encode_batch_ragged, tables
 *             of 32*srcs*rows bytes; a read that rebuilds fewer than `rows`
 *             columns leaves the other rows unreferenced
 *  src_dptrs / src_nblocks: HOST arrays [num_reads][srcs]: the parts of the
 *             slice that the read uses, by the ragged call's rules — address
 *             of block 0's data and block count; source j has block b iff
 *             b < its count, beyond that it counts as zeros and no byte of
 *             it is read; a slot of count 0 may have address 0.  The counts
 *             of a short chunk's parts (slice_traits.h:311-316) are how the
 *             chunk's end is expressed: there is no chunk length.
 *  view_parts : ks, the data parts of the slice, 1..32; one value per call.
 *             Chunk block c is row c / ks, column c % ks.
 *  col_map    : HOST array [num_reads][ks], where a column comes from:
 *             j < srcs   = source slot j, copied;
 *             0x80 + r, r < rows = lost, and equal to table row r applied to
 *                          the read's sources (XOR_j tbl[r][j] * src_j[row],
 *                          absent sources skipped);
 *             0xFF       = unmapped, legal only if no requested block of the
 *                          read falls in the column.
 *             No slot and no row may stand for two columns of one read.
 *  first_block / block_count / dst_dptrs: HOST arrays [num_reads]: output
 *             block i < block_count is chunk block first_block + i, 65536
 *             bytes at dst + i*dst_block_stride.  A range may start and end
 *             anywhere inside a row.  A requested block that none of its
 *             sources reaches (at or past the chunk's end) is written as
 *             zeros, as SliceReadPlan::postProcessRead pads
 *             (slice_read_plan.h:94-105).
 *  src_block_stride / dst_block_stride: as for the strided call; a
 *             dst_block_stride above 65536 leaves the bytes between two
 *             output blocks (the CRC slots of an INTERLEAVED image) alone
 * Only the counted source blocks are read — and of those only the ones a
 * row needs: a row without a lost requested column reads just its requested
 * columns.  Only the requested output blocks are written.  An output must
 * not overlap any source or other output of the call.
 * One launch per pass of 8 table rows (one launch at rows == 0); one
 * workgroup per tile of every (read, block row) that a range touches loads
 * each source tile once, stores it to the output block of the column it
 * backs and accumulates it into the lost columns' rows
 * (csrc/ec_kernel_read.h).  Copies happen in the first pass only.
 * Scratch cost, device and pinned host each: per read 20 bytes, 16 bytes per
 * source slot and 4 per table row, plus 8 bytes per (read, block row); per
 * call the tables (32*srcs*rows*ntables bytes) and up to 15 bytes of padding
 * behind each of seven sections.  A whole-chunk ec(8,2) read (128 block
 * rows) takes about 1.2 KiB.  Kept with the stream's scratch as for the
 * gates.
 * Returns LIZEC_EINVAL from the host, with nothing enqueued and no output
 * byte written, for everything the ragged call refuses about sources, tables
 * (at rows > 0) and strides; view_parts or srcs outside 1..32, rows outside
 * 0..32; a col_map value that names a slot >= srcs or a row >= rows, or a
 * slot or row named twice; a requested column that is unmapped, or mapped to
 * a slot of address 0; block_count == 0 or first_block + block_count >
 * 1048576; a destination address that is 0 or not a multiple of 4; a NULL
 * array; num_reads < 1; or (read, block row) pairs times 8 above 2^31-1.
 * A side whose stride and used addresses are all multiples of 16 keeps the
 * aligned vector accesses.  There is no plan form.  Stream and thread
 * contract as for the other batch calls. */
int lizec_chunk_read_batch(lizec_engine *e, int srcs, int rows,
                           const uint8_t *gftbls, int ntables,
                           const uint32_t *tbl_index,
                           const uint64_t *src_dptrs,
                           const uint32_t *src_nblocks, int view_parts,
                           const uint8_t *col_map, const uint32_t *first_block,
                           const uint32_t *block_count,
                           const uint64_t *dst_dptrs, int num_reads,
                           uint32_t src_block_stride,
                           uint32_t dst_block_stride, void *stream);

/* The same read on the host: the addresses are HOST addresses and no GPU is
 * needed (memcpy for the copied columns, ec_encode_data over the present
 * sources for the lost ones).  Same refusals (nothing written), same bytes. */
int lizec_chunk_read_host(int srcs, int rows, const uint8_t *gftbls,
                          int ntables, const uint32_t *tbl_index,
                          const uint64_t *src_ptrs,
                          const uint32_t *src_nblocks, int view_parts,
                          const uint8_t *col_map, const uint32_t *first_block,
                          const uint32_t *block_count,
                          const uint64_t *dst_ptrs, int num_reads,
                          uint32_t src_block_stride,
                          uint32_t dst_block_stride);

/* The VERIFIED chunk read — lizec_chunk_read_batch with the check that the
 * reference's client makes before it decodes anything: every received 64 KiB
 * block is compared with the CRC that came with it
 * (ReadOperationExecutor, read_operation_executor.cc:261-263:
 * mycrc32(0, block, MFSBLOCKSIZE)), and a part with a bad block is recorded
 * (ChunkReader::readData, chunk_reader.cc:135-137, crcErrors_) so that the
 * next plan leaves it out (:63-65).  Every argument up to dst_block_stride
 * is lizec_chunk_read_batch's, with the same meaning.
 *  crc_dptrs  : HOST array [num_reads][srcs]: device address of the CRC of
 *             the slot's block 0, any alignment; 0 = the slot is not
 *             verified (it is copied and used as it is).
 *  crc_block_stride: >= 4; the CRC of the slot's block b is the 4 bytes,
 *             big-endian, at crc + b*crc_block_stride.  4 for a CRC array
 *             (MooseFS header order); 65540 with crc = data - 4 for an
 *             INTERLEAVED image or a stream of whole-block READ_DATA packets
 *             (what lizec_read_gate_batch emits).
 *  dev_bad_out: device u32[num_reads]: bit j is set iff a checked block of
 *             slot j failed.  Every entry is written, 0 for a clean read.
 * Which blocks are checked: block b of slot j iff the slot has a CRC
 * address, b < src_nblocks[read][j], and the read loads the block — the
 * column the slot backs is requested in row b, or some lost column is.  A
 * row without a lost requested column thus checks just its requested
 * columns, a row with one checks every present slot, and blocks at or past
 * a part's count are never checked.  Each such block is checked exactly
 * once; of any other block no data byte and no CRC byte is read.  There is
 * no sparse-block rule (a stored CRC of 0 is compared like any other): that
 * rule is the chunkserver's (hddspacemgr.cc:1556-1596).
 * Order on the stream: dev_bad_out is zeroed, the verify kernel runs (one
 * wave per (read, block row, slot), hash only: csrc/read_verify.h), then
 * exactly the launches of lizec_chunk_read_batch.  The output bytes are
 * therefore written WHETHER OR NOT a check fails — the verdict is known only
 * after the pass, as for the read gate.  THE CALLER MUST DISCARD THE OUTPUT
 * OF A READ WHOSE MASK IS NOT 0, drop the flagged parts and read again.
 * Scratch cost: that of lizec_chunk_read_batch plus 8 bytes per source slot
 * (the CRC addresses, staged behind the destination addresses), device and
 * pinned host each: 24 bytes per source slot in all.
 * Returns LIZEC_EINVAL from the host, with nothing enqueued and no byte
 * written (dev_bad_out included), for everything lizec_chunk_read_batch
 * refuses, a NULL crc_dptrs or dev_bad_out, or crc_block_stride < 4.
 * Stream and thread contract as for the other batch calls. */
int lizec_chunk_read_verified_batch(
    lizec_engine *e, int srcs, int rows, const uint8_t *gftbls, int ntables,
    const uint32_t *tbl_index, const uint64_t *src_dptrs,
    const uint32_t *src_nblocks, int view_parts, const uint8_t *col_map,
    const uint32_t *first_block, const uint32_t *block_count,
    const uint64_t *dst_dptrs, int num_reads, uint32_t src_block_stride,
    uint32_t dst_block_stride, const uint64_t *crc_dptrs,
    uint32_t crc_block_stride, uint32_t *dev_bad_out, void *stream);

/* The same on the host: every address is a HOST address, bad_out a host
 * array u32[num_reads]; lizec_crc32 over the same blocks by the same rule,
 * then lizec_chunk_read_host.  Same refusals (nothing written), same bytes,
 * same masks. */
int lizec_chunk_read_verified_host(
    int srcs, int rows, const uint8_t *gftbls, int ntables,
    const uint32_t *tbl_index, const uint64_t *src_ptrs,
    const uint32_t *src_nblocks, int view_parts, const uint8_t *col_map,
    const uint32_t *first_block, const uint32_t *block_count,
    const uint64_t *dst_ptrs, int num_reads, uint32_t src_block_stride,
    uint32_t dst_block_stride, const uint64_t *crc_ptrs,
    uint32_t crc_block_stride, uint32_t *bad_out);

/* The CLIENT WRITE of an EC or xor slice: ChunkWriter::startOperation
 * (mount/chunk_writer.cc:475-547) with computeParityBlock (:365-402) and the
 * CRCs of WriteExecutor::addDataPacket (write_executor.cc:91-107), for a
 * batch of writes in one call.
 *
 * The slice has view_parts = ks data parts (the columns of
 * lizec_chunk_read_batch) and `rows` parity parts; chunk block c is row
 * c / ks, column c % ks.  One write carries the new bytes [from, to) —
 * size = to - from, the same range of every block (Operation::
 * isExpandPossible, :57-71) — of chunk blocks [first_block, first_block +
 * block_count).  For every block row b that the range touches, column c is,
 * as `size` bytes,
 *   - the new data, if chunk block b*ks + c lies in the range;
 *   - else bytes [from, to) of block b of the data part behind column c as
 *     it is now (fillStripe, :440-466) — a "fill";
 *   - else zeros, if that part has no block b (:451, reed_solomon.h:79);
 * and parity r of row b is row r of gftbls applied to those ks columns.
 * gftbls is 32*ks*rows bytes, [row][column][32], one table per call:
 * lizec_rs_encode_tables(k, m) for ec(k,m), ec_init_tables over ones for a
 * xor slice.  Only [from, to) of anything is read or written.  The data
 * packets are the caller's own bytes; the device work is the parity and the
 * CRC of every packet, lizec_crc32(0, bytes, size). */
typedef struct lizec_chunk_write {   /* 40 bytes, no padding */
	uint64_t data;        /* address of the size bytes for block first_block;
	                         block first_block+i at data + i*data_stride; any
	                         alignment */
	uint64_t crcs;        /* u32 array, 4-byte aligned, or 0 = no CRCs wanted */
	uint32_t data_stride; /* >= size; unused if block_count == 1 */
	uint32_t par_stride;  /* >= size; unused if the range touches one row */
	uint32_t first_block, block_count;
	uint32_t from, to;    /* 0 <= from < to <= 65536 */
} lizec_chunk_write;

/*  fill_dptrs[w][c], fill_nblocks[w][c]: address of block 0's data and block
 *      count of the data part behind column c, by the ragged call's rules
 *      (a count of 0 may come with address 0); the counts express the
 *      chunk's current end.  Block b is read at fill + b*fill_block_stride +
 *      from, only in rows the write touches and only for columns the range
 *      does not cover there; a write of whole rows may pass all counts as 0.
 *  fill_block_stride: >= 65536 (65536 MooseFS, 65540 INTERLEAVED).
 *  par_dptrs[w][r]: address of the first byte written for parity r of the
 *      FIRST touched row r0 = first_block / ks; row r0 + i goes to
 *      + i*par_stride, size bytes each.  In place in an image: image block 0
 *      + r0*stride + from, par_stride = the image's stride; a packet staging
 *      buffer: its start, par_stride = size.  Any alignment.  0 = this
 *      parity part is not wanted: nothing is computed for it and its CRC
 *      slots are not written.
 *  crcs[i], i < block_count: CRC of new block i; crcs[block_count + i*rows +
 *      r]: CRC of parity r of touched row i; host order.
 * Exactly the size bytes of each wanted parity row and the CRC slots are
 * written.  Loads touch only aligned 16-byte units that hold a byte of a
 * range.  A parity output must not overlap a data range, a fill range or
 * another output of the call, and two writes that touch the same row do not
 * belong in one call (canStartOperation, :345-355).  An operation with a hole
 * inside a row is passed as its covering range.  Every fill column must be
 * readable; a slice with lost parts is written through
 * lizec_chunk_write_degraded_batch below.
 * Returns LIZEC_EINVAL from the host, with nothing enqueued and no byte
 * written, for a NULL array; num_writes < 1; rows or view_parts outside
 * 1..32; from >= to or to > 65536; block_count == 0 or first_block +
 * block_count > 1048576; a data address of 0; a stride below size where the
 * stride is used; fill_block_stride < 65536; a fill count above 32768, or a
 * nonzero fill count with address 0; a crcs address that is not a multiple
 * of 4; all parities of a write unwanted while crcs is 0; more than 2^31-1
 * workgroups in a pass (one per 16 KiB tile of every touched row where a pass
 * has up to 4 parities, per 8 KiB tile otherwise), or more than 2^24 CRCs.  A call in which every used address,
 * every used stride, every `from` and every size is a multiple of 16 takes
 * the aligned vector form.  Stream, thread and scratch contract as for the
 * other batch calls. */
int lizec_chunk_write_batch(lizec_engine *e, int rows, const uint8_t *gftbls,
                            const lizec_chunk_write *writes, int num_writes,
                            const uint64_t *fill_dptrs,
                            const uint32_t *fill_nblocks, int view_parts,
                            uint32_t fill_block_stride,
                            const uint64_t *par_dptrs, void *stream);

/* The same on the host: HOST addresses, no GPU.  Same refusals (nothing
 * written), same bytes. */
int lizec_chunk_write_host(int rows, const uint8_t *gftbls,
                           const lizec_chunk_write *writes, int num_writes,
                           const uint64_t *fill_ptrs,
                           const uint32_t *fill_nblocks, int view_parts,
                           uint32_t fill_block_stride,
                           const uint64_t *par_ptrs);

/* The CLIENT WRITE into a slice with lost parts.  ChunkWriter::fillStripe
 * (mount/chunk_writer.cc:440-466) fills a partly written row through
 * readBlocks (:557-615), a planned read over whichever parts have a
 * location, so a lost data part is rebuilt from the survivors before the
 * parity is computed.  Rebuild and encode are both linear over GF(2^8): they
 * fold into one coefficient table over "new columns + old sources", and one
 * pass reads every needed byte range once and nothing outside [from, to).
 *
 * lizec_degraded_write_table builds that table for one row shape of ec(k,m),
 * or of a xor slice of k data parts (is_xor != 0, m = 1: an all-ones
 * generator; parts are numbered as ec's here, data 0..k-1, the parity k).
 *  new_mask  : the data columns that are NEW in the row
 *  have_mask : the data columns whose part has this block row (not ABSENT)
 *  avail_mask: the parts, data and parity, that can be read as they are now
 *  slot_part : [srcs], the part behind each old-source slot, each part at
 *              most once
 *  gftbl     : out, 32*(k+srcs)*m bytes, [m][k + srcs][32] in
 *              gf_vect_mul_init format: column c < k multiplies new column
 *              c, column k + j the old bytes of slot j
 *  use_mask  : out, the slots whose column is not all zero
 * A column of have & ~new whose part is available is a plain fill with
 * coefficient G[r,c].  One that is not is rebuilt from the first k available
 * parts, ascending (ec_read_plan.h:126-133; for xor, all the others), by the
 * inversion lizec_rs_tables uses, and the products G[r,c] * R[c,s] are
 * folded into the survivors' columns: the table gives, bit for bit, what
 * rebuilding first and encoding second gives.  A surviving data part outside
 * have_mask counts as zeros: it is not used and needs no slot.  A row without
 * a lost fill
 * column comes out as the healthy table, use_mask exactly its fill columns.
 * For a xor slice the coefficients cancel (1 ^ 1 = 0) to the
 * read-modify-write form new ^ old ^ old parity, and the cancelled slots
 * are not in use_mask.
 * Returns LIZEC_EINVAL for k, m outside 1..32, srcs outside 1..32, a NULL
 * array, is_xor with m != 1, a mask bit outside the slice, a slot naming a
 * part outside the slice or one named before, a part that is needed (a
 * readable fill column; a survivor that is a parity part or lies in
 * have_mask) without a slot, and a lost fill column with fewer than k parts available ("Not
 * enough chunkservers to read full data"); LIZEC_ESINGULAR as
 * lizec_rs_tables. */
int lizec_degraded_write_table(int k, int m, int is_xor, uint32_t new_mask,
                               uint32_t have_mask, uint64_t avail_mask,
                               const uint8_t *slot_part, int srcs,
                               uint8_t *gftbl, uint32_t *use_mask);

/* lizec_chunk_write_batch over such tables.  The writes, par_dptrs (0 = not
 * wanted: how a lost parity part is expressed), par_stride, the CRC slots
 * and their order, the passes, the scratch and the stream and thread
 * contract are lizec_chunk_write_batch's.  Instead of fill columns there are
 *  srcs (1..32) old-source slots: old_dptrs[w][j], old_nblocks[w][j], by the
 *      ragged call's rules; a slot is a part, data or parity.  Slot j is
 *      present in row b iff b < old_nblocks[w][j], and is then read at old +
 *      b*old_block_stride + from, size bytes, any alignment;
 *  gftbls: ntables tables of 32*(view_parts+srcs)*rows bytes each,
 *      [row][view_parts + srcs][32]; use_masks[ntables] their slot masks;
 *  tbl_index[w][3]: the table of the write's first touched row, of the rows
 *      between (all NEW; its mask should be 0, but the call just obeys the
 *      mask) and of its last touched row where that is not the first.
 * Parity r of row b is the XOR of tbl[r][c] * new_c over the columns NEW in
 * the row and of tbl[r][view_parts + j] * old_j over the slots that are in
 * the table's mask and present.  A slot outside the mask, or at or past its
 * count, is neither loaded nor addressed.
 * An output must not overlap a data range, an old-source range or another
 * output of the call.  In particular a parity part that serves as an old
 * source cannot be written in place by the same call (the unaligned load
 * forms read neighbouring lanes' dwords, so an update in place would race):
 * stage that parity as packets (par_stride = size) and apply them behind
 * the call.
 * Returns LIZEC_EINVAL from the host, with nothing enqueued and no byte
 * written, for everything lizec_chunk_write_batch refuses (read "old" for
 * "fill"), and for srcs outside 1..32; ntables < 1; a table index >=
 * ntables; a mask bit >= srcs; a nonzero count with address 0 on a slot
 * that is in the mask of a table of a row the write touches.  Where the
 * healthy call speaks of fill addresses, for the refusal as for the aligned
 * form, read: the addresses of those slots; a slot outside those masks is
 * never addressed, whatever it holds. */
int lizec_chunk_write_degraded_batch(
    lizec_engine *e, int rows, const uint8_t *gftbls, int ntables,
    const uint32_t *use_masks, const uint32_t *tbl_index,
    const lizec_chunk_write *writes, int num_writes,
    const uint64_t *old_dptrs, const uint32_t *old_nblocks, int srcs,
    int view_parts, uint32_t old_block_stride, const uint64_t *par_dptrs,
    void *stream);

/* The same on the host: HOST addresses, no GPU, ec_encode_data per row over
 * the view_parts + srcs candidates.  Same refusals (nothing written), same
 * bytes. */
int lizec_chunk_write_degraded_host(
    int rows, const uint8_t *gftbls, int ntables, const uint32_t *use_masks,
    const uint32_t *tbl_index, const lizec_chunk_write *writes, int num_writes,
    const uint64_t *old_ptrs, const uint32_t *old_nblocks, int srcs,
    int view_parts, uint32_t old_block_stride, const uint64_t *par_ptrs);

/* Per-block CRC32 over a contiguous device buffer:
 *  dev_crcs_out[b] = lizec_crc32(seed, dev_buf + b*block_len, block_len)
 * The chunkserver's per-64KiB-block gate (hddspacemgr.cc:1918-1920, scrub
 * :2148-2212, replicate chunk_replicator.cc:189) in batch form.
 *  block_len: a multiple of 1024, below 2^27 (128 MiB): the combine step
 *             appends zero runs of up to block_len/2 bytes, and its matrix
 *             bank covers runs shorter than 2^26
 *  dev_buf  : at least 4-byte aligned.  16-byte aligned buffers take the
 *             vector-load kernels; 4- and 8-byte aligned ones (INTERLEAVED
 *             chunk format) are read with dword loads at every block_len
 * Anything else returns LIZEC_EINVAL from the host; nothing is enqueued
 * and dev_crcs_out is not written. */
int lizec_crc32_batch(lizec_engine *e, const void *dev_buf, uint32_t block_len,
                      uint64_t nblocks, uint32_t seed, uint32_t *dev_crcs_out,
                      void *stream);

/* CRC32 of n independent byte ranges:
 *  dev_crcs_out[i] = lizec_crc32(seed, dptrs[i], lens[i])
 * The ranges hdd_write hashes (hddspacemgr.cc:1918, :1951-1953) and the
 * client's write path produces (write_executor.cc:94-102): any length up to
 * a block, at any byte address.  One launch per call, one wave per range.
 *  dptrs : HOST array of n device addresses, of ANY byte alignment
 *  lens  : HOST array of n lengths, 0..65536 (the reference's
 *          LIZARDFS_ERROR_WRONGSIZE bound); a length of 0 gives `seed`, and
 *          its address is not used and may be 0
 *  dev_crcs_out: device u32[n], host-order values as for lizec_crc32_batch
 * Ranges may overlap or repeat.  No byte outside [dptrs[i], dptrs[i] +
 * lens[i]) is read: the bytes before the first and behind the last 16-byte
 * boundary inside a range are loaded one at a time, the aligned middle in
 * 16-byte vectors (folded 16 bytes per step from the first whole aligned
 * unit on; csrc/crc_ranges.h).  The launch has at most 16384 workgroups of
 * 4 waves; beyond 65536 ranges every wave takes several.
 * Returns LIZEC_EINVAL from the host, with nothing enqueued and
 * dev_crcs_out not written, for a NULL array, n == 0 or n > 2^24, a length
 * above 65536, or a non-zero length with address 0.  Stream and thread
 * contract as for the other batch calls (the tables travel through the
 * stream's call scratch). */
int lizec_crc32_ranges(lizec_engine *e, const uint64_t *dptrs,
                       const uint32_t *lens, uint32_t n, uint32_t seed,
                       uint32_t *dev_crcs_out, void *stream);

/* Batched chunk scrub — hdd_int_test semantics (hddspacemgr.cc:2148-2212)
 * over MooseFS-format chunk-part images (chunk.cc:126-188: 1 KiB signature
 * block, big-endian u32 CRC array at crc_off, 64 KiB blocks at data_off):
 * verifies every block's CRC against the stored array.
 *  chunk_dptrs[i] : device address of part-file image i
 *  data_offs[i]   : header size (offset of block 0)
 *  crc_offs[i]    : offset of the CRC array (kMaxSignatureBlockSize = 1024)
 *  block_counts[i]: blocks in image i
 *  dev_status_out : device int32[nchunks]; first damaged block index, or
 *                   INT32_MAX if the image is clean. */
int lizec_scrub_batch(lizec_engine *e, const uint64_t *chunk_dptrs,
                      const uint32_t *data_offs, const uint32_t *crc_offs,
                      const uint32_t *block_counts, int nchunks,
                      int32_t *dev_status_out, void *stream);

/* Generalized layout: block b's data at data_offs[i] + b*block_stride,
 * its stored CRC at crc_offs[i] + b*crc_stride.  Covers both on-disk
 * formats: MooseFS (stride 65536 / 4; the wrapper above) and INTERLEAVED
 * (kHddBlockSize = 65540, chunk.h:40: 4-byte CRC inline before each
 * block — data_off 4, both strides 65540, crc_off 0).  Block data must be
 * 4-byte aligned (chunk_dptrs[i] + data_offs[i] and block_stride multiples
 * of 4) and block_stride >= 65536; the stored CRC is read bytewise and needs
 * no alignment.  The largest block count times either stride must not exceed
 * 2^32-1.  Anything else, a NULL array, an address of 0 (also for an image
 * of no blocks), or no blocks at all returns LIZEC_EINVAL with nothing
 * enqueued; dev_status_out is not written. */
int lizec_scrub_batch_strided(lizec_engine *e, const uint64_t *chunk_dptrs,
                              const uint32_t *data_offs,
                              const uint32_t *crc_offs,
                              const uint32_t *block_counts, int nchunks,
                              uint32_t block_stride, uint32_t crc_stride,
                              int32_t *dev_status_out, void *stream);

/* The store counterpart of lizec_scrub_batch_strided: computes the CRC of
 * every 64 KiB block (at data_offs[i] + b*block_stride) and STORES it
 * big-endian at crc_offs[i] + b*crc_stride; no other byte of an image is
 * written.  Arguments as above, without the status array.  Block data must
 * be 4-byte aligned (chunk_dptrs[i] + data_offs[i] and block_stride
 * multiples of 4) and block_stride >= 65536, and the largest block count
 * times either stride must not exceed 2^32-1; anything else, a NULL array,
 * an address of 0, or no blocks at all returns LIZEC_EINVAL with nothing
 * enqueued.  The two calls share these checks. */
int lizec_crc_fill_batch_strided(lizec_engine *e, const uint64_t *chunk_dptrs,
                                 const uint32_t *data_offs,
                                 const uint32_t *crc_offs,
                                 const uint32_t *block_counts, int nchunks,
                                 uint32_t block_stride, uint32_t crc_stride,
                                 void *stream);

/* The batched write gate — what hdd_write (hddspacemgr.cc:1899-2009) checks
 * and computes before it touches the disk, for n writes at once.  One op is
 * one packet: `size` bytes for [offset, offset + size) of one 64 KiB block. */
typedef struct lizec_write_op {   /* 40 bytes, no padding */
	uint64_t data;    /* device address of the `size` bytes to write */
	uint64_t block;   /* device address of the block's current 65536 bytes;
	                     0 = block at or past the end of the chunk */
	uint64_t stored;  /* device address of the block's stored CRC, 4 bytes
	                     big-endian, read bytewise (as the scrub does) */
	uint32_t offset, size;
	uint32_t crc;     /* the CRC the client claims for data */
	uint32_t reserved;/* 0 */
} lizec_write_op;

enum { LIZEC_GATE_OK = 0, LIZEC_GATE_BAD_DATA = 1, LIZEC_GATE_BAD_BLOCK = 2 };
enum { LIZEC_GATE_SPARSE = 1 };

/* Per op, line for line after hdd_write:
 *  - crc != crc32(0, data, size): LIZEC_GATE_BAD_DATA (:1918); nothing else
 *    decides that op's outputs.
 *  - offset == 0 && size == 65536: newcrc = crc (:1922-1941); block and
 *    stored are ignored and may be 0.
 *  - partial write, block == 0: the block counts as zeros (:1973-1991),
 *    pre = zeroblock(0, offset), post = zeroblock(0, 65536-offset-size); no
 *    stored CRC is read.
 *  - partial write, block != 0: pre, changed and post are the CRCs of
 *    block[0, offset), block[offset, offset+size) and the rest, combined as
 *    :1954-1962 does (lizec_crc32_splice, with its offset == 0 branch and
 *    the post step skipped when the range ends the block); a result other
 *    than the stored CRC gives LIZEC_GATE_BAD_BLOCK (:1965).
 *  - flags & LIZEC_GATE_SPARSE: a block whose four stored bytes are zero
 *    and whose 65536 bytes are all zero (tested on the bytes, not by CRC)
 *    counts as stored = zeroblock(0, 65536) — the INTERLEAVED read path's
 *    rule (hddspacemgr.cc:1779, crc.cc:235-243).  Without the flag it does
 *    not apply (MooseFS format, :1751).
 *  - on LIZEC_GATE_OK, newcrc = splice(pre, offset, crc, size, post, 65536)
 *    (:1992-2001); otherwise newcrc = 0.  size == 0 is legal and comes out
 *    as the same algebra gives.
 * The gate writes nothing but its two outputs: copying the data in and
 * storing newcrc stay with the caller.
 *  ops            : HOST array of n ops
 *  dev_status_out : device int32[n], LIZEC_GATE_*
 *  dev_newcrc_out : device u32[n]
 * Two launches: lizec_crc32_ranges' kernel over four range slots per op
 * (data, pre, changed, post; a slot an op does not need has length 0),
 * carrying an OR of the bytes it reads for the sparse rule, then a
 * finishing kernel, one thread per op, that combines, compares and writes
 * the outputs.  The ranges are hashed before any data CRC is known, so the
 * block of an op that ends as BAD_DATA is read too.  Op and range tables
 * travel through the stream's call scratch; stream and thread contract as
 * for the other batch calls.
 * Scratch cost: 120 bytes of device scratch and 88 bytes of pinned host
 * staging per op.  Both grow by doubling and stay with the stream's scratch
 * until the engine is destroyed, so choose n by that and not by the bound
 * below: 2^24 ops in one call hold about 2 GiB of each, 2^16 ops 8 MiB of
 * each.  (lizec_crc32_ranges: 12 bytes of each per range.)
 * Returns LIZEC_EINVAL from the host, with nothing enqueued and the outputs
 * not written, for a NULL array, n == 0 or n > 2^24, size > 65536,
 * offset >= 65536, offset + size > 65536, reserved != 0, size > 0 with
 * data == 0, a partial op with block != 0 and stored == 0, or an unknown
 * flag bit. */
int lizec_write_gate_batch(lizec_engine *e, const lizec_write_op *ops,
                           uint32_t n, uint32_t flags,
                           int32_t *dev_status_out, uint32_t *dev_newcrc_out,
                           void *stream);

/* The same gate on the host: the addresses in ops are HOST addresses, the
 * outputs host arrays, and no GPU is needed.  Same refusals (outputs not
 * written), same results bit for bit. */
int lizec_write_gate_host(const lizec_write_op *ops, uint32_t n,
                          uint32_t flags, int32_t *status, uint32_t *newcrc);

/* The batched read gate — what hdd_read (hddspacemgr.cc:1662-1727) does
 * with one block through hdd_read_crc_and_block (:1525-1608), for n reads at
 * once.  One op is one READ of `size` bytes at `offset` inside one 64 KiB
 * block; its result is the payload of cstocl READ_DATA:
 * [4-byte big-endian CRC][the bytes]. */
typedef struct lizec_read_op {   /* 32 bytes, no padding */
	uint64_t block;   /* device address of the block's 65536 bytes;
	                     0 = block at or past the end of the chunk */
	uint64_t stored;  /* address of its stored CRC, 4 bytes big-endian, read
	                     bytewise */
	uint64_t out;     /* address of the packet: 4 + size bytes are written */
	uint32_t offset, size;
} lizec_read_op;

/* Per op, line for line after hdd_read / hdd_read_crc_and_block:
 *  - block == 0 (:1535-1541, blocknum >= c->blocks): the packet's CRC is
 *    zeroblock(0, size) — emptyblockcrc for a whole block — and its data
 *    `size` zero bytes; status LIZEC_GATE_OK; stored is ignored.
 *  - otherwise have = the CRC of block[0, 65536), spliced (as
 *    lizec_crc32_splice does) from pre = block[0, offset),
 *    mid = block[offset, offset + size) and post = the rest.
 *    Without LIZEC_GATE_SPARSE (MooseFS format, :1547-1555): stored != have
 *    gives LIZEC_GATE_BAD_BLOCK (the reference's ERROR_CRC).
 *    With LIZEC_GATE_SPARSE (INTERLEAVED format, :1556-1596): a block whose
 *    four stored bytes are all zero is NOT checked (:1571-1587 never calls
 *    checkCRC there); its CRC counts as emptyblockcrc if its 65536 bytes
 *    are all zero (tested on the bytes, not by CRC) and as 0 otherwise.
 *    Stored bytes that are not all zero are checked as for MooseFS.
 *  - on LIZEC_GATE_OK the packet's CRC is the block's CRC as just
 *    determined when offset == 0 && size == 65536 (:1711-1712 passes the
 *    stored value through, recomputing nothing), and crc32(0, block +
 *    offset, size) for any other range (:1718); the data is the range.
 *  - on LIZEC_GATE_BAD_BLOCK the four CRC bytes are written as 0 and the
 *    data bytes as read: the reference, too, copies before it checks, and
 *    the verdict is known only after the pass.  Send no such packet.
 * Nothing outside [out, out + 4 + size) and dev_status_out[i] is written;
 * no byte outside [block, block + 65536) and the four stored bytes is read.
 * block and out may have ANY byte alignment.  Blocks may overlap or repeat
 * between ops; packets must not overlap each other or any block or stored
 * CRC of the call — otherwise the result is undefined.
 *  ops            : HOST array of n ops
 *  flags          : 0 or LIZEC_GATE_SPARSE, for the whole call
 *  dev_status_out : device int32[n], LIZEC_GATE_OK or LIZEC_GATE_BAD_BLOCK
 * One launch: one wave per op reads the block once, hashing pre, mid and
 * post, storing mid to out + 4 from the registers it is hashed from, then
 * splices, compares and writes CRC bytes and status (csrc/read_gate.h).  The
 * stores are 16 bytes wide when (out + 4 - block - offset) is a multiple of
 * 16, 16-byte vectors at 4-byte alignment when it is a multiple of 4, single
 * bytes otherwise: a packet that is itself 16-byte aligned takes the second
 * form for a 16-byte aligned block; align out + 4 with block + offset for
 * the first.  At most 16384 workgroups of 4 waves; beyond 65536 ops every
 * wave takes several.  The op table travels through the stream's call
 * scratch; stream and thread contract as for the other batch calls.
 * Scratch cost: 32 bytes of device scratch and 32 bytes of pinned host
 * staging per op, kept with the stream's scratch as for the write gate.
 * Returns LIZEC_EINVAL from the host, with nothing enqueued and no output
 * written, for a NULL array, n == 0 or n > 2^24, size == 0 or offset + size
 * > 65536 (hdd_read's ERROR_WRONGSIZE, :1669), offset >= 65536, out == 0,
 * block != 0 with stored == 0, or an unknown flag bit. */
int lizec_read_gate_batch(lizec_engine *e, const lizec_read_op *ops,
                          uint32_t n, uint32_t flags, int32_t *dev_status_out,
                          void *stream);

/* The same gate on the host: the addresses in ops are HOST addresses, status
 * a host array, and no GPU is needed.  Same refusals (nothing written), same
 * packets and status bit for bit. */
int lizec_read_gate_host(const lizec_read_op *ops, uint32_t n, uint32_t flags,
                         int32_t *status);

/* Pinned host memory for the streaming APIs (hipHostMalloc/hipHostFree):
 * pageable buffers work too but degrade the pipeline to synchronous
 * copies. */
int lizec_host_alloc(void **ptr, uint64_t bytes);
void lizec_host_free(void *p);

/* Streaming chunk rebuild — ChunkReplicator::replicate
 * (chunk_replicator.cc:139-196) as a host-to-host pipeline: H2D the
 * surviving parts, EC-recover the erased parts, CRC every recovered
 * 64 KiB block (chunk_replicator.cc:189), assemble complete MooseFS part
 * images (chunk.cc:126-188: signature bytes at 0, big-endian CRC array at
 * crc_off, blocks at header_size) and D2H them — double-buffered over two
 * streams so H2D/compute/D2H overlap.
 *  part_len    : bytes per part, multiple of 65536
 *  ic, oc      : surviving parts in / parts to rebuild per chunk
 *  gftbls      : 32*ic*oc recover tables (lizec_rs_tables)
 *  host_src    : nchunks*ic HOST addresses of surviving part bytes
 *  sigs        : nchunks*oc signatures (sig_len bytes each), or NULL
 *  header_size : image header bytes; crc_off: CRC array offset within it
 *  host_dst    : nchunks*oc HOST addresses, header_size+part_len each
 *  sub_batch   : chunks per pipeline stage (0 = auto: 2 GiB of device
 *                staging per slot, at most 64 chunks; clamped to nchunks)
 * Returns LIZEC_EINVAL from the host, with nothing allocated or enqueued
 * and no byte of the destinations written, for a NULL e, gftbls, host_src
 * or host_dst, nchunks < 1, ic or oc outside 1..32, part_len 0, not a
 * multiple of 65536 or above 2^31, sig_len > header_size, a CRC array that
 * does not fit in the header (crc_off + 4*(part_len/65536) > header_size),
 * or a header_size that is not a multiple of 16: the images are staged
 * back to back and their blocks, header_size in, are read and written with
 * 16-byte vector accesses (every real header is a multiple of 1024,
 * chunk.cc getHeaderSize).  sigs == NULL or sig_len == 0 leaves the
 * signature block zero.  Exactly header_size + part_len bytes are written
 * at every destination address and part_len read at every source address;
 * the addresses are otherwise unrelated (any row stride on either side). */
int lizec_replicate_run(lizec_engine *e, uint64_t part_len, int ic, int oc,
                        const uint8_t *gftbls, const uint64_t *host_src,
                        const uint8_t *sigs, uint32_t sig_len,
                        uint32_t header_size, uint32_t crc_off,
                        const uint64_t *host_dst, int nchunks, int sub_batch);

/* The same pipeline emitting INTERLEAVED-format images (chunk.cc:191-209),
 * for a chunkserver that does not create chunks in MooseFS format: no
 * header and no signature; block b's big-endian CRC at 65540*b and its
 * data right behind it.  Recovery writes straight into the images through
 * the strided EC kernel.
 *  host_dst : nchunks*oc HOST addresses, (part_len/65536)*65540 bytes each
 * Everything else as for lizec_replicate_run. */
int lizec_replicate_run_interleaved(lizec_engine *e, uint64_t part_len, int ic,
                                    int oc, const uint8_t *gftbls,
                                    const uint64_t *host_src,
                                    const uint64_t *host_dst, int nchunks,
                                    int sub_batch);

/* Streaming rebuild of chunks of ANY length and erasure pattern, sources
 * verified: lizec_replicate_run with a block count per source and per
 * destination of every chunk and a recover table per chunk — the job of
 * ChunkReplicator::replicate as the reference does it, which asks each chunk
 * for its own block count (chunk_replicator.cc:142-145), plans it from
 * whatever parts are available (SliceRecoveryPlanner::prepare, :168) and
 * checks every block it receives against the CRC that came with it
 * (read_operation_executor.cc:261-263).
 *  gftbls, ntables, tbl_index: as for lizec_ec_encode_batch_ragged;
 *             tbl_index is a HOST array [nchunks] or NULL = table 0
 *  host_src / src_nblocks: HOST arrays [nchunks][ic]: source j of chunk c is
 *             src_nblocks[c][j] plain 64 KiB blocks, back to back at HOST
 *             address host_src[c][j].  Blocks at or past a source's count are
 *             the zeros past the chunk's end: not read, not copied, and they
 *             need no buffer; an address whose count is 0 may be 0
 *  host_src_crc: NULL, or a HOST array [nchunks][ic] of HOST addresses: the
 *             source's CRC array, one big-endian CRC per block, 4 bytes
 *             apart, at any alignment — what a MooseFS-format part file holds
 *             at offset 1024 and what the replicator collects from its
 *             READ_DATA packets.  0 = that slot is not verified.  Every block
 *             below the source's count is hashed on the GPU after it lands
 *             (csrc/replicate_stage.h) and compared; nothing past the count
 *             is read, neither a data byte nor a CRC byte
 *  bad_out  : HOST array [nchunks]; bit j of bad_out[c] is set iff a block
 *             of source j of chunk c failed its check, 0 otherwise; complete
 *             when the call returns.  The images are emitted either way (as
 *             in lizec_chunk_read_verified_batch): a chunk whose mask is not
 *             0 must be discarded.  Required with host_src_crc; without it
 *             it may be NULL, and is zeroed if given
 *  host_dst / dst_nblocks: HOST arrays [nchunks][oc]: destination l of chunk
 *             c is an image of its own size at HOST address host_dst[c][l]:
 *               MooseFS (flags 0): header_size + dst_nblocks*65536 bytes,
 *                 signature at 0, the rest of the header zero, big-endian
 *                 CRCs at crc_off, blocks at header_size — what
 *                 lizec_replicate_run emits;
 *               LIZEC_REPL_INTERLEAVED: dst_nblocks*65540 bytes, each block
 *                 behind its CRC; sigs, sig_len, header_size and crc_off are
 *                 unused.
 *             A nonzero address with count 0 is a header-only MooseFS image,
 *             or nothing at all in INTERLEAVED format.  Address 0 with count
 *             0: the slot is not wanted.  Exactly the image's bytes are
 *             written at each address.  A run in which no destination has a
 *             block is legal and emits headers only
 *  sigs     : nchunks*oc signatures (sig_len bytes each), or NULL = zeros
 *  stage_bytes: device staging per pipeline slot; 0 = 2 GiB, what
 *             lizec_replicate_run's auto sizing uses.  There are two slots.
 *             The run is cut into stages by lizec_replicate_ragged_stages and
 *             the slots are sized for the largest one
 * Each stage runs in stream order on its slot's own stream: H2D of the
 * sources into a packed arena, H2D of the stage's metadata (tables' index,
 * block maps, counts, addresses, signatures and the sources' CRC bytes, one
 * pinned block), one header kernel, the verify kernel if asked, the ragged
 * EC kernel straight into the images, the CRC fill with per-image counts,
 * D2H of each image and of the stage's masks.  Zero-length copies are
 * skipped.  All scratch lives in the slots and is freed before the call
 * returns; the engine's per-stream scratch is not used.
 * Returns LIZEC_EINVAL from the host, with nothing allocated or enqueued and
 * no byte of the destinations or of bad_out written, for a NULL e, gftbls,
 * host_src, src_nblocks, host_dst or dst_nblocks, nchunks < 1, ic or oc
 * outside 1..32, a tbl_index entry >= ntables, ntables outside the limits of
 * the multi call, a count above 1024, a nonzero count with address 0,
 * bad_out == NULL with host_src_crc != NULL, an unknown flag bit,
 * stage_bytes above 2^31, more block rows in the run than
 * lizec_ragged_block_map accepts, and for MooseFS images a header_size that
 * is not a multiple of 16, sig_len > header_size or a CRC array that does
 * not fit (crc_off + 4*max(dst_nblocks) > header_size).  Use
 * lizec_host_alloc'd buffers for real overlap; pageable ones stay correct. */
#define LIZEC_REPL_INTERLEAVED 1u   /* images in INTERLEAVED format; else MooseFS */
int lizec_replicate_run_ragged(
    lizec_engine *e, int ic, int oc, const uint8_t *gftbls, int ntables,
    const uint32_t *tbl_index, const uint64_t *host_src,
    const uint32_t *src_nblocks, const uint64_t *host_src_crc,
    const uint8_t *sigs, uint32_t sig_len, uint32_t header_size,
    uint32_t crc_off, const uint64_t *host_dst, const uint32_t *dst_nblocks,
    int nchunks, uint64_t stage_bytes, uint32_t flags, uint32_t *bad_out);

/* The stage cut of lizec_replicate_run_ragged (pure host, no GPU; the GPU
 * call uses exactly this function).  A chunk's footprint is its source bytes
 * (counts * 65536) plus the bytes of its wanted images (host_dst != 0), each
 * image rounded up to 16.  A stage takes chunks in order while the sum of
 * their footprints stays within stage_bytes (0 = 2 GiB); a chunk that alone
 * exceeds stage_bytes is a stage of its own.
 *  stage_first: receives stages + 1 entries — stage i is chunks
 *             [stage_first[i], stage_first[i + 1]) — or NULL to count only
 *  cap      : room in stage_first, in entries
 * Returns the number of stages, or LIZEC_EINVAL for a NULL array, nchunks
 * < 1, ic or oc outside 1..32, a count above 1024, an unknown flag bit,
 * stage_bytes above 2^31, or stages + 1 > cap. */
int64_t lizec_replicate_ragged_stages(
    int ic, int oc, const uint32_t *src_nblocks, const uint64_t *host_dst,
    const uint32_t *dst_nblocks, int nchunks, uint32_t header_size,
    uint32_t flags, uint64_t stage_bytes, uint32_t *stage_first,
    uint64_t cap);

/* The same rebuild on the host, byte for byte, images and bad_out: the
 * no-GPU floor of the path.  Same arguments without e and stage_bytes, same
 * refusals (nothing written). */
int lizec_replicate_ragged_host(
    int ic, int oc, const uint8_t *gftbls, int ntables,
    const uint32_t *tbl_index, const uint64_t *host_src,
    const uint32_t *src_nblocks, const uint64_t *host_src_crc,
    const uint8_t *sigs, uint32_t sig_len, uint32_t header_size,
    uint32_t crc_off, const uint64_t *host_dst, const uint32_t *dst_nblocks,
    int nchunks, uint32_t flags, uint32_t *bad_out);

#ifdef __cplusplus
}
#endif

#endif /* LIZEC_H */
